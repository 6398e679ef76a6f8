"""Vocabulary layers: ``IntegerLookup`` and ``StringLookup`` on a device-resident hash table.

The reference's tutorials put ``tf.keras.layers.StringLookup(vocabulary=..., mask_token=None)`` or
``tf.keras.layers.IntegerLookup(vocabulary=..., mask_value=None)`` in front of every ``Embedding``.  Keras is
not part of the reference tree, so the rules below are the contract of these layers.

Index layout: index 0 is the mask token when ``mask_token`` is not ``None``; the ``num_oov_indices`` OOV slots
come next; the vocabulary follows in order.  An unknown integer ``x`` maps to OOV slot
``floormod(x, num_oov_indices)``, an unknown string to ``fingerprint mod num_oov_indices`` (unsigned).  With
``num_oov_indices=0`` an unknown id maps to ``-1`` and the call stays asynchronous; ``forward(...,
validate=True)`` reads a device counter afterwards and raises ``ValueError`` (Keras always raises; this layer
does not pay a host synchronisation on the hot path).

The table (``csrc/vocab.hip``) is open addressing with linear probing over 16-byte ``{key, value}`` slots,
built on the device with a 64-bit compare-and-swap per token (which also finds repeated keys) and probed by
one lane per id.  A lookup launches one kernel, allocates nothing but its output and never synchronises, so
it can sit inside a captured step.

``StringLookup`` is the same integer table over 64-bit SipHash-2-4 fingerprints of the UTF-8 bytes
(``tfrs_fingerprint_bytes``).  Two vocabulary strings with equal fingerprints raise ``ValueError`` in
``set_vocabulary``; an unknown string whose fingerprint equals a token's is taken for that token (chance
2^-64 per pair).  Keras's own FarmHash is out of scope, as it is for ``Hashing``.

The vocabulary is the persistent state (``state_dict()`` / ``load_state_dict()``); the table is rebuilt on
load, never stored.
"""

import collections
from typing import List, Optional

import numpy as np
import torch

from recommenders_amd import _lib
from recommenders_amd.layers.hashing import _device, pack_strings
from recommenders_amd.layers.tpu_embedding_layer import RaggedIds, SparseIds

EMPTY_KEY = -(1 << 63)        # TFRS_VOCAB_EMPTY_KEY: marks a free slot, never stored in the table
_DUPLICATE_KEY, _TABLE_FULL = 1, 2


def table_capacity(n: int) -> int:
  """Slots of the table of ``n`` tokens: the power of two >= 2 n (at least 2)."""
  cap = 2
  while cap < 2 * n:
    cap *= 2
  return cap


def _as_bytes(x) -> bytes:
  """UTF-8 bytes of a token; surrogate escapes (``get_vocabulary`` of a token that is not UTF-8) go back to bytes."""
  return bytes(x) if isinstance(x, (bytes, np.bytes_)) else str(x).encode("utf-8", "surrogateescape")


def _string_array(x) -> np.ndarray:
  """Lists become object arrays: NumPy's own conversion would decode ``bytes`` next to ``str`` as ASCII."""
  return x if isinstance(x, np.ndarray) else np.array(x, dtype=object)


def _is_batch(x) -> bool:
  return isinstance(x, (torch.Tensor, np.ndarray, RaggedIds, SparseIds))


def _batches(data):
  """``adapt``'s argument as a sequence of batches: one tensor / array / flat list is one batch."""
  if _is_batch(data) or isinstance(data, (str, bytes)):
    return [data]
  if isinstance(data, (list, tuple)):
    return list(data) if any(_is_batch(x) or isinstance(x, (list, tuple)) for x in data) else [data]
  return data   # any other iterable yields batches


def _values_of(batch):
  return batch.values if isinstance(batch, (RaggedIds, SparseIds)) else batch


class _IndexLookup(torch.nn.Module):
  """What both layers share: the index layout, the table and the lookup launch over int64 keys."""

  _oov_unsigned = 0

  def __init__(self, max_tokens, num_oov_indices, mask_token, oov_token, invert, output_mode, device, mask_value):
    super().__init__()
    if mask_value is not None:
      if mask_token is not None and mask_token != mask_value:
        raise ValueError("`mask_value` is an alias of `mask_token`; pass one of them")
      mask_token = mask_value
    if output_mode != "int":
      raise NotImplementedError(f"output_mode={output_mode!r}: only 'int' is on the hot path")
    if int(num_oov_indices) < 0:
      raise ValueError(f"`num_oov_indices` must be >= 0; got {num_oov_indices}")
    if max_tokens is not None and int(max_tokens) <= 1:
      raise ValueError(f"`max_tokens` must be greater than 1; got {max_tokens}")
    self.max_tokens = None if max_tokens is None else int(max_tokens)
    self.num_oov_indices = int(num_oov_indices)
    self.mask_token = mask_token
    self.oov_token = oov_token
    self.invert = bool(invert)
    self.output_mode = output_mode
    self._device = device
    self._table = None         # [capacity, 2] int64 on the GPU
    self._n_tokens = 0
    self._empty_value = -1     # vocabulary position of the token whose key is EMPTY_KEY, if any
    self._mask_key = 0
    self._unknown = None       # device counter of validate=True
    if mask_token is not None and mask_token == oov_token:
      raise ValueError(f"`mask_token` and `oov_token` must differ; both are {mask_token!r}")

  # ---- index layout ----------------------------------------------------------------------------
  @property
  def _has_mask(self) -> int:
    return 0 if self.mask_token is None else 1

  @property
  def _base(self) -> int:
    return self._has_mask + self.num_oov_indices

  def _special_tokens(self) -> list:
    return [self.mask_token] * self._has_mask + [self.oov_token] * self.num_oov_indices

  def vocabulary_size(self) -> int:
    return self._base + self._n_tokens

  def _check_size(self, n_tokens: int) -> None:
    if self.max_tokens is not None and self._base + n_tokens > self.max_tokens:
      raise ValueError(f"the vocabulary has {self._base + n_tokens} entries with its {self._base} special "
                       f"tokens, more than max_tokens={self.max_tokens}")

  # ---- table -----------------------------------------------------------------------------------
  def _build_table(self, keys: torch.Tensor) -> None:
    """keys[n] int64 on the GPU -> the table; repeated keys raise ValueError."""
    n = keys.numel()
    cap = table_capacity(n)
    table = torch.empty((cap, 2), dtype=torch.int64, device=keys.device)
    flags = torch.empty((1,), dtype=torch.int32, device=keys.device)
    _lib.check(_lib.load().tfrs_vocab_build(_lib.ptr(keys), n, _lib.ptr(table), cap, _lib.ptr(flags),
                                            _lib.current_stream()))
    at_empty = (keys == EMPTY_KEY).nonzero().reshape(-1)
    flag = int(flags.item())
    if flag & _DUPLICATE_KEY or at_empty.numel() > 1:
      raise ValueError(self._duplicate_message())
    if flag & _TABLE_FULL:
      raise RuntimeError("vocabulary table: a token found no free slot")
    self._table, self._n_tokens = table, n
    self._empty_value = int(at_empty[0]) if at_empty.numel() else -1
    self._unknown = torch.zeros((1,), dtype=torch.int64, device=keys.device)

  def _require_table(self) -> torch.Tensor:
    if self._table is None:
      self.set_vocabulary([])
    return self._table

  def _lookup_keys(self, keys: torch.Tensor, validate: bool) -> torch.Tensor:
    table = self._require_table()
    flat = keys.to(table.device).reshape(-1).contiguous()
    out = torch.empty(flat.shape, dtype=torch.int64, device=table.device)
    if validate:
      self._unknown.zero_()
    _lib.check(_lib.load().tfrs_vocab_lookup(
        _lib.ptr(flat), 1 if flat.dtype == torch.int64 else 0, flat.numel(), _lib.ptr(table), table.shape[0],
        self._n_tokens, self._base, self._has_mask, self._mask_key, self._empty_value, self._has_mask,
        self.num_oov_indices, self._oov_unsigned, _lib.ptr(self._unknown if validate else None), _lib.ptr(out),
        _lib.current_stream()))
    if validate and self.num_oov_indices == 0:
      unknown = int(self._unknown.item())
      if unknown:
        raise ValueError(f"{unknown} of {flat.numel()} ids are not in the vocabulary and "
                         "num_oov_indices=0 leaves no index for them")
    return out.reshape(keys.shape)

  def forward(self, inputs, validate: bool = False):
    if isinstance(inputs, RaggedIds):
      return inputs.with_values(self.forward(inputs.values, validate))
    if isinstance(inputs, SparseIds):
      return SparseIds(inputs.indices, self.forward(inputs.values, validate), inputs.dense_shape)
    return self._invert(inputs) if self.invert else self._lookup(inputs, validate)

  # ---- persistence: the vocabulary, not the table ----------------------------------------------
  def get_extra_state(self):
    return {"vocabulary": self._state_tokens()}

  def set_extra_state(self, state):
    self.set_vocabulary(state["vocabulary"])

  def adapt(self, data):
    """Builds the vocabulary from data: a tensor or array, or an iterable of batches.  Tokens are ordered by
    count descending, ties by token descending, and cut to ``max_tokens`` minus the special slots; mask and
    OOV tokens in the data are not counted."""
    tokens = self._count_order(_batches(data))
    if self.max_tokens is not None:
      tokens = tokens[:max(self.max_tokens - self._base, 0)]
    self.set_vocabulary(tokens)


class IntegerLookup(_IndexLookup):
  """``tf.keras.layers.IntegerLookup``: int32 / int64 ids of any shape -> int64 indices on the GPU."""

  def __init__(self, max_tokens: Optional[int] = None, num_oov_indices: int = 1, mask_token: Optional[int] = None,
               oov_token: int = -1, vocabulary=None, invert: bool = False, output_mode: str = "int",
               device: Optional[torch.device] = None, mask_value: Optional[int] = None):
    super().__init__(max_tokens, num_oov_indices, None if mask_token is None else int(mask_token), int(oov_token),
                     invert, output_mode, device, None if mask_value is None else int(mask_value))
    self._tokens = torch.empty((0,), dtype=torch.int64)
    self._inverse = None
    if vocabulary is not None:
      self.set_vocabulary(vocabulary)

  def _duplicate_message(self) -> str:
    return "the vocabulary contains repeated tokens"

  def set_vocabulary(self, vocabulary) -> None:
    """``vocabulary``: a list, array or tensor of integers.  A host vocabulary is checked for repeats on the
    host; a vocabulary that already lives on the GPU is checked by the build's compare-and-swap alone."""
    if isinstance(vocabulary, torch.Tensor):
      vocab = vocabulary.detach()
    else:
      arr = np.asarray(vocabulary if len(vocabulary) else [], dtype=None if len(vocabulary) else np.int64)
      vocab = torch.from_numpy(np.ascontiguousarray(arr))
    if vocab.dtype.is_floating_point or vocab.dtype == torch.bool or vocab.dtype.is_complex:
      raise ValueError(f"IntegerLookup needs an integer vocabulary; got {vocab.dtype}")
    vocab = vocab.reshape(-1).long()
    special = self._special_tokens()
    k = len(special)
    if k and vocab.numel() >= k and vocab[:k].tolist() == special:
      vocab = vocab[k:]
    for name, token in (("mask", self.mask_token), ("OOV", self.oov_token)):
      if token is not None and bool((vocab == token).any()):
        raise ValueError(f"the reserved {name} token {token} is only accepted at its own leading position "
                         "of the vocabulary")
    self._check_size(vocab.numel())
    if not vocab.is_cuda and torch.unique(vocab).numel() != vocab.numel():
      raise ValueError(self._duplicate_message())
    keys = vocab.to(_device(self._device)).contiguous()
    self._mask_key = 0 if self.mask_token is None else self.mask_token
    self._build_table(keys)
    self._tokens = keys
    head = torch.tensor(special, dtype=torch.int64, device=keys.device)
    self._inverse = torch.cat([head, keys])

  def get_vocabulary(self, include_special_tokens: bool = True) -> List[int]:
    return (self._special_tokens() if include_special_tokens else []) + self._tokens.tolist()

  def _state_tokens(self):
    return self._tokens.cpu()

  def _count_order(self, batches) -> torch.Tensor:
    flat = []
    for batch in batches:
      values = _values_of(batch)
      t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
      if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"IntegerLookup needs integer input; got {t.dtype}")
      flat.append(t.reshape(-1).long())
    if not flat:
      return torch.empty((0,), dtype=torch.int64)
    data = torch.cat([t.to(flat[0].device) for t in flat])
    keep = data != self.oov_token
    if self.mask_token is not None:
      keep &= data != self.mask_token
    tokens, counts = torch.unique(data[keep], return_counts=True)   # tokens ascending
    tokens, counts = tokens.flip(0), counts.flip(0)
    return tokens[torch.sort(counts, descending=True, stable=True).indices]

  def _as_ids(self, inputs) -> torch.Tensor:
    if not isinstance(inputs, torch.Tensor):
      arr = np.asarray(inputs)
      if arr.dtype.kind not in ("i", "u"):
        raise ValueError(f"IntegerLookup needs integer input; got dtype {arr.dtype}")
      inputs = torch.as_tensor(arr.astype(np.int64))
    if inputs.dtype not in (torch.int32, torch.int64):
      if inputs.dtype.is_floating_point or inputs.dtype == torch.bool:
        raise ValueError(f"IntegerLookup needs integer input; got {inputs.dtype}")
      inputs = inputs.long()
    return inputs

  def _lookup(self, inputs, validate: bool) -> torch.Tensor:
    return self._lookup_keys(self._as_ids(inputs), validate)

  def _invert(self, inputs) -> torch.Tensor:
    """Indices -> tokens, an int64 tensor on the GPU; OOV slots and out-of-range indices give ``oov_token``."""
    self._require_table()
    idx = self._as_ids(inputs).to(self._inverse.device).long()
    size = self._inverse.numel()
    inside = (idx >= 0) & (idx < size)
    if size == 0:
      return torch.full_like(idx, self.oov_token)
    return torch.where(inside, self._inverse[idx.clamp(0, size - 1)], torch.full_like(idx, self.oov_token))


class StringLookup(_IndexLookup):
  """``tf.keras.layers.StringLookup``: arrays or lists of ``str`` / ``bytes`` -> int64 indices on the GPU.

  A string is known by the 64-bit SipHash-2-4 fingerprint of its UTF-8 bytes: an unknown string whose
  fingerprint equals a token's is taken for that token (chance 2^-64 per pair)."""

  _oov_unsigned = 1

  def __init__(self, max_tokens: Optional[int] = None, num_oov_indices: int = 1, mask_token: Optional[str] = None,
               oov_token: str = "[UNK]", vocabulary=None, invert: bool = False, output_mode: str = "int",
               device: Optional[torch.device] = None, mask_value: Optional[str] = None):
    super().__init__(max_tokens, num_oov_indices, None if mask_token is None else _as_bytes(mask_token),
                     _as_bytes(oov_token), invert, output_mode, device,
                     None if mask_value is None else _as_bytes(mask_value))
    self._tokens: List[bytes] = []
    if vocabulary is not None:
      self.set_vocabulary(vocabulary)

  def _duplicate_message(self) -> str:
    return "the vocabulary contains repeated tokens, or two tokens with the same 64-bit fingerprint"

  def _fingerprints(self, strings, dev: torch.device) -> torch.Tensor:
    arr = np.empty(len(strings), dtype=object)
    arr[:] = [_as_bytes(x) for x in strings]
    d_blob, d_off = pack_strings(arr, dev)
    out = torch.empty((len(strings),), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().tfrs_fingerprint_bytes(_lib.ptr(d_blob), _lib.ptr(d_off), len(strings), _lib.ptr(out),
                                                  _lib.current_stream()))
    return out

  def set_vocabulary(self, vocabulary) -> None:
    """``vocabulary``: a list or array of ``str`` or ``bytes``."""
    arr = _string_array(vocabulary).reshape(-1)
    if any(not isinstance(x, (str, bytes, np.str_, np.bytes_)) for x in arr):
      raise ValueError("StringLookup needs a vocabulary of str or bytes")
    vocab = [_as_bytes(x) for x in arr]
    special = self._special_tokens()
    k = len(special)
    if k and len(vocab) >= k and vocab[:k] == special:
      vocab = vocab[k:]
    for name, token in (("mask", self.mask_token), ("OOV", self.oov_token)):
      if token is not None and token in vocab:
        raise ValueError(f"the reserved {name} token {token!r} is only accepted at its own leading position "
                         "of the vocabulary")
    self._check_size(len(vocab))
    if len(set(vocab)) != len(vocab):
      raise ValueError("the vocabulary contains repeated tokens")
    dev = _device(self._device)
    prints = self._fingerprints(([self.mask_token] if self._has_mask else []) + vocab, dev)
    keys = prints[self._has_mask:]
    if self._has_mask:
      self._mask_key = int(prints[0])
      if bool((keys == self._mask_key).any()):
        raise ValueError("a vocabulary token has the mask token's 64-bit fingerprint")
    self._build_table(keys.contiguous())
    self._tokens = vocab

  def get_vocabulary(self, include_special_tokens: bool = True) -> List[str]:
    tokens = (self._special_tokens() if include_special_tokens else []) + self._tokens
    return [t.decode("utf-8", "surrogateescape") for t in tokens]

  def _state_tokens(self):
    return list(self._tokens)

  def _count_order(self, batches) -> List[bytes]:
    counts = collections.Counter()
    for batch in batches:
      values = _values_of(batch)
      counts.update(_as_bytes(x) for x in _string_array(values).reshape(-1))
    counts.pop(self.oov_token, None)
    if self.mask_token is not None:
      counts.pop(self.mask_token, None)
    by_token = sorted(counts, reverse=True)                       # UTF-8 bytes descending
    return sorted(by_token, key=lambda t: -counts[t])             # stable: count descending

  def _lookup(self, inputs, validate: bool) -> torch.Tensor:
    if isinstance(inputs, torch.Tensor):
      raise ValueError(f"StringLookup needs string input; got a tensor of {inputs.dtype}")
    arr = _string_array(inputs)
    if arr.dtype.kind not in ("U", "S", "O") or (arr.dtype.kind == "O" and not all(
        isinstance(x, (str, bytes)) for x in arr.reshape(-1))):
      raise ValueError(f"StringLookup needs string input; got dtype {arr.dtype}")
    table = self._require_table()
    return self._lookup_keys(self._fingerprints(arr.reshape(-1), table.device).reshape(arr.shape), validate)

  def _invert(self, inputs) -> np.ndarray:
    """Indices -> tokens, a NumPy array of ``str`` on the host; OOV slots and out-of-range indices give
    ``oov_token``."""
    idx = inputs.detach().cpu().numpy() if isinstance(inputs, torch.Tensor) else np.asarray(inputs)
    if idx.dtype.kind not in ("i", "u"):
      raise ValueError(f"StringLookup(invert=True) needs integer indices; got dtype {idx.dtype}")
    names = np.array(self.get_vocabulary() + [self.oov_token.decode("utf-8", "surrogateescape")], dtype=object)
    oov = len(names) - 1
    idx = idx.astype(np.int64)
    return names[np.where((idx >= 0) & (idx < oov), idx, oov)]
