"""NumPy / dict restatement of IntegerLookup and StringLookup, and a Python restatement of the table of
``csrc/vocab.hip`` (no test functions; imported by ``test_vocab_host.py`` and ``test_vocab_gpu.py``).

The rules are those of the layers' contract: index 0 is the mask token when there is one,
the OOV slots follow, then the vocabulary in order; an unknown integer goes to ``floormod(x, num_oov)``, an
unknown string to ``fingerprint mod num_oov`` (unsigned), and with no OOV slot to ``-1``.  ``adapt`` orders
tokens by count descending, ties by token descending, and cuts the list to ``max_tokens`` minus the special
slots.  The SipHash fingerprint comes from ``oracle/hashing.py``.
"""

import collections

import numpy as np

from oracle import hashing as o_hash

U64 = (1 << 64) - 1
EMPTY_KEY = -(1 << 63)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
FINGERPRINT_KEY = (0x0706050403020100, 0x0F0E0D0C0B0A0908)   # key bytes 00 01 .. 0f


# ---- the layers --------------------------------------------------------------------------------
def layout(mask_token, num_oov):
  """(index of the first OOV slot, index of the first vocabulary token)."""
  has_mask = 0 if mask_token is None else 1
  return has_mask, has_mask + num_oov


def vocabulary_size(vocabulary, mask_token, num_oov):
  return layout(mask_token, num_oov)[1] + len(vocabulary)


def integer_lookup(ids, vocabulary, mask_token=None, num_oov=1):
  ids = np.asarray(ids)
  oov_base, base = layout(mask_token, num_oov)
  index = {int(t): base + i for i, t in enumerate(vocabulary)}
  out = np.empty(ids.size, dtype=np.int64)
  for j, x in enumerate(ids.reshape(-1).tolist()):
    if mask_token is not None and x == mask_token:
      out[j] = 0
    elif x in index:
      out[j] = index[x]
    else:
      out[j] = oov_base + x % num_oov if num_oov else -1     # Python's % is floormod
  return out.reshape(ids.shape)


def as_bytes(x):
  return bytes(x) if isinstance(x, (bytes, np.bytes_)) else str(x).encode("utf-8")


def fingerprint(x):
  """Unsigned 64-bit SipHash-2-4 of the UTF-8 bytes under the fixed key."""
  return o_hash.siphash24(FINGERPRINT_KEY[0], FINGERPRINT_KEY[1], as_bytes(x))


def as_signed(u):
  return u - (1 << 64) if u >= (1 << 63) else u


def string_lookup(strings, vocabulary, mask_token=None, num_oov=1):
  arr = strings if isinstance(strings, np.ndarray) else np.array(strings, dtype=object)
  oov_base, base = layout(mask_token, num_oov)
  index = {as_bytes(t): base + i for i, t in enumerate(vocabulary)}
  out = np.empty(arr.size, dtype=np.int64)
  for j, s in enumerate(arr.reshape(-1)):
    b = as_bytes(s)
    if mask_token is not None and b == as_bytes(mask_token):
      out[j] = 0
    elif b in index:
      out[j] = index[b]
    else:
      out[j] = oov_base + fingerprint(b) % num_oov if num_oov else -1
  return out.reshape(arr.shape)


def adapt_order(batches, mask_token, oov_token, num_oov=1, max_tokens=None, strings=False):
  """The vocabulary ``adapt`` builds from ``batches`` (lists of tokens)."""
  counts = collections.Counter()
  for batch in batches:
    for x in np.asarray(batch, dtype=object).reshape(-1):
      counts[as_bytes(x) if strings else int(x)] += 1
  for special in (mask_token, oov_token):
    if special is not None:
      counts.pop(as_bytes(special) if strings else int(special), None)
  tokens = sorted(counts, key=lambda t: (-counts[t], _descending(t)))
  if max_tokens is not None:
    tokens = tokens[:max(max_tokens - layout(mask_token, num_oov)[1], 0)]
  return tokens


class _descending:
  """Sort key that reverses the order of ints or of byte strings."""

  def __init__(self, token):
    self.token = token

  def __lt__(self, other):
    return self.token > other.token

  def __eq__(self, other):
    return self.token == other.token


def inverse(indices, vocabulary, mask_token, oov_token, num_oov=1):
  full = [mask_token] * (mask_token is not None) + [oov_token] * num_oov + list(vocabulary)
  return [full[i] if 0 <= i < len(full) else oov_token for i in np.asarray(indices).reshape(-1).tolist()]


# ---- the table ---------------------------------------------------------------------------------
def mix(x):
  """The kernel's slot mixer: MurmurHash3's 64-bit finalizer."""
  x &= U64
  x ^= x >> 33
  x = (x * 0xFF51AFD7ED558CCD) & U64
  x ^= x >> 33
  x = (x * 0xC4CEB9FE1A85EC53) & U64
  x ^= x >> 33
  return x


def mix_array(x):
  x = np.asarray(x).astype(np.uint64)
  x = x ^ (x >> np.uint64(33))
  x = x * np.uint64(0xFF51AFD7ED558CCD)
  x = x ^ (x >> np.uint64(33))
  x = x * np.uint64(0xC4CEB9FE1A85EC53)
  return x ^ (x >> np.uint64(33))


def home(key, capacity):
  return mix(key) & (capacity - 1)


def capacity_for(n):
  cap = 2
  while cap < 2 * n:
    cap *= 2
  return cap


def keys_homed_at(slot, capacity, count, start=1, exclude=()):
  """The first ``count`` integers >= ``start`` (not in ``exclude``) whose home slot at ``capacity`` is ``slot``."""
  found, lo, skip = [], start, set(exclude)
  while len(found) < count:
    x = np.arange(lo, lo + (1 << 22), dtype=np.int64)
    hits = x[(mix_array(x) & np.uint64(capacity - 1)) == np.uint64(slot)]
    found.extend(int(h) for h in hits.tolist() if h not in skip)
    lo += 1 << 22
  return found[:count]


class ProbeTable:
  """Open addressing, linear probing, ``capacity`` slots {key, value}; keys inserted in list order."""

  def __init__(self, keys, capacity=None):
    self.capacity = capacity_for(len(keys)) if capacity is None else capacity
    assert self.capacity & (self.capacity - 1) == 0 and self.capacity >= 2 * len(keys)
    self.keys = [EMPTY_KEY] * self.capacity
    self.values = [-1] * self.capacity
    self.empty_value = -1
    self.duplicate = False
    for i, key in enumerate(keys):
      if key == EMPTY_KEY:
        self.duplicate |= self.empty_value >= 0
        self.empty_value = i
        continue
      slot = home(key, self.capacity)
      for _ in range(self.capacity):
        if self.keys[slot] == EMPTY_KEY:
          self.keys[slot], self.values[slot] = key, i
          break
        if self.keys[slot] == key:
          self.duplicate = True
          break
        slot = (slot + 1) & (self.capacity - 1)

  def lookup(self, key):
    """(value or -1, probe steps taken)."""
    if key == EMPTY_KEY:
      return self.empty_value, 0
    slot = home(key, self.capacity)
    for step in range(self.capacity):
      if self.keys[slot] == key:
        return self.values[slot], step + 1
      if self.keys[slot] == EMPTY_KEY:
        return -1, step + 1
      slot = (slot + 1) & (self.capacity - 1)
    return -1, self.capacity

  def occupied(self):
    return sorted(s for s in range(self.capacity) if self.keys[s] != EMPTY_KEY)


# ---- hand-built cases (shared by the host and the GPU suites) -------------------------------------
def chain_case():
  """Eight tokens homed at slot 13 of a capacity-16 table (the chain wraps to slots 0..4) and the absent
  queries: homed at 13, homed inside the chain (slots 14, 15, 0, 2, 4) and homed at free slots (5, 9, 12)."""
  tokens = keys_homed_at(13, 16, 8)
  absent_home = keys_homed_at(13, 16, 4, exclude=tokens)
  absent_chain = [keys_homed_at(s, 16, 1)[0] for s in (14, 15, 0, 2, 4)]
  absent_free = [keys_homed_at(s, 16, 1)[0] for s in (5, 9, 12)]
  return tokens, absent_home, absent_chain, absent_free
