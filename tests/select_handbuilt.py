"""Hand-built lists for the top-K selection layer (csrc/topk_select.hip: ``select_kernel<KP>`` with its dense, parts and
expand sources; csrc/topk_api.hip: ``exclude_kernel``): every builder returns the arrays of one call of a C entry point
(``tfrs_topk_update_from_scores``, ``tfrs_topk_merge`` / ``_strided``, ``tfrs_topk_expand_duplicates``,
``tfrs_topk_exclude``) together with the list the call must return, so a test compares the result slot by slot instead
of through a whole layer on a random corpus, which cannot steer how often a wave's ``chunk`` fills, which of the two
dense walks a row takes, where the row tail lies or whether a state arrives short.

The restated order is the one ``make_key`` (csrc/common.h) defines -- score descending, ``-0.0`` ties with ``+0.0``,
lower row first on ties, a row below 0 does not exist -- as a ``numpy.lexsort`` over (row, -score) without any
floating-point arithmetic.  Selection only moves bit patterns: every comparison is bit for bit, scores as uint32.
``select_kernel`` returns ``+0.0`` for a ``-0.0`` input (the key is canonicalised) and ``(0.0, -1)`` in empty slots;
``exclude_kernel`` copies the original bits.

The dense walk's offer order and the ``consume`` / ``absorb_chunk`` bookkeeping are restated as well (``dense_offers``,
``simulate``): tests/test_select_handbuilt_host.py uses them to prove what each case reaches.  Pure numpy at import; the
``device_*`` functions import torch when they are called.  Test infrastructure only."""

import numpy as np

KS = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)      # both sides of every KP switch of launch_select
MAX_K = 1024
NEG_ZERO = np.uint32(0x80000000)
INF = np.float32(np.inf)
TOP_ROW = 0x7FFFFFFF
SENTINEL = 0x5A5A5A5A                                          # int32 fill of the guard rows around every output
INF_BITS = np.uint32(0x7F800000)
POISON_ROW = 3                                                 # the (valid) row number of every poisoned slot


def kp_of(k):
  for kp in (64, 128, 256, 512):
    if k <= kp:
      return kp
  return 1024


# ------------------------------------------------------------------------------------------ the order, restated
def bits(scores):
  return np.ascontiguousarray(scores, np.float32).view(np.uint32)


def canonical_bits(scores):
  """uint32 patterns with -0.0 turned into +0.0 (what a key keeps of a score)."""
  b = bits(scores).copy()
  b[b == NEG_ZERO] = 0
  return b


def restated_order(scores, rows):
  """Positions of the existing entries (row >= 0) in result order: score descending, row ascending on ties."""
  scores, rows = np.asarray(scores, np.float32).ravel(), np.asarray(rows, np.int64).ravel()
  keep = np.flatnonzero(rows >= 0)
  return keep[np.lexsort((rows[keep], -scores[keep]))]


def restated_topk(scores, rows, k):
  """(score bits uint32 [k], rows int32 [k]) of the top k of one query's entries; empty slots are (0.0, -1)."""
  scores, rows = np.asarray(scores, np.float32).ravel(), np.asarray(rows, np.int64).ravel()
  order = restated_order(scores, rows)[:k]
  out_s, out_r = np.zeros(k, np.uint32), np.full(k, -1, np.int32)
  out_s[:order.size] = canonical_bits(scores[order])
  out_r[:order.size] = rows[order]
  return out_s, out_r


# ------------------------------------------------------------------------------------------ keys and the walk, restated
def make_keys(scores, rows):
  """The 64-bit keys of csrc/common.h (host model only; the expected lists do not use them)."""
  b = canonical_bits(scores)
  hi = np.where(b & NEG_ZERO, ~b, b | NEG_ZERO).astype(np.uint64)
  lo = (~np.asarray(rows, np.int64)) & 0xFFFFFFFF
  return (hi << np.uint64(32)) | lo.astype(np.uint64)


def dense_offers(nb, aligned):
  """The dense walk as a list of offers, each an int64 [64] of columns (-1: the lane offers nothing).  Aligned rows walk
  2048 scores per batch (8 x 64 lanes x 4) as whole 16-byte pieces -- lanes past the last whole piece re-read it and
  drop it -- then ``nb % 4`` scalars; other rows walk 64 columns at a time."""
  lane = np.arange(64, dtype=np.int64)
  out = []
  if not aligned:
    for base in range(0, nb, 64):
      e = base + lane
      out.append(np.where(e < nb, e, -1))
    return out
  n4 = nb & ~3
  for base in range(0, n4, 2048):
    for u in range(8):
      if base + u * 256 < n4:
        e = base + (u * 64 + lane) * 4
        for c in range(4):
          out.append(np.where(e + 4 <= n4, e + c, -1))
  if n4 < nb:
    e = n4 + lane
    out.append(np.where(e < nb, e, -1))
  return out


def simulate(k, offers_keys, state_keys=()):
  """``consume`` / ``absorb_chunk`` of one wave: ``offers_keys`` is a list of uint64 [64] (0 = nothing offered),
  ``state_keys`` the seeded entries.  Returns (best keys [k], log) where log lists, per absorb, (index of the offer that
  triggered it or None for the one after the walk, fill at that moment), plus ``touch``: the offers that found
  ``fill + 64 == KP`` with something to add and did not absorb."""
  kp = kp_of(k)
  best = np.zeros(kp, np.uint64)
  best[:len(state_keys)] = np.sort(np.asarray(state_keys, np.uint64))[::-1]
  chunk, fill, kth = [], 0, best[k - 1]
  absorbs, touch, passed = [], [], []

  def absorb():
    nonlocal best, chunk
    best = np.sort(np.concatenate([best, np.asarray(chunk, np.uint64)]))[::-1][:kp]
    chunk = []

  for n, keys in enumerate(offers_keys):
    p = keys > kth
    cnt = int(p.sum())
    passed.append(cnt)
    if cnt == 0:
      continue
    if fill + 64 > kp:
      absorbs.append((n, fill))
      absorb()
      fill, kth = 0, best[k - 1]
    elif fill + 64 == kp:
      touch.append(n)
    chunk.extend(keys[p].tolist())
    fill += cnt
  if fill > 0:
    absorbs.append((None, fill))
    absorb()
  return best[:k], dict(absorbs=absorbs, touch=touch, passed=passed)


def keys_to_lists(keys):
  """(score bits, rows) of a key array as the kernel writes them."""
  keys = np.asarray(keys, np.uint64)
  u = (keys >> np.uint64(32)).astype(np.uint32)
  b = np.where(u & NEG_ZERO, u ^ NEG_ZERO, ~u).astype(np.uint32)
  rows = (~keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
  empty = keys == 0
  return np.where(empty, np.uint32(0), b), np.where(empty, np.int32(-1), rows)


# ------------------------------------------------------------------------------------------ a. dense rows
DENSE_NB = (1, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 2052, 4099, 6151)
PATTERNS = ("planted", "ascending", "descending", "equal", "tieblocks", "zeros", "infs")


def planted_positions(nb):
  """Where the dense walk can drop or double a score: the first and the last 16-byte piece of every 2048-score batch,
  the last whole piece (re-read at a clamped address by every lane past the end) and each tail scalar."""
  n4 = nb & ~3
  pos = dict(batch_first=[], batch_last=[], last_piece=list(range(max(n4 - 4, 0), n4)), tail=list(range(n4, nb)))
  for base in range(0, n4, 2048):
    pos["batch_first"] += list(range(base, min(base + 4, n4)))
    if base + 2048 <= n4:
      pos["batch_last"] += list(range(base + 2044, base + 2048))
  return pos


def all_planted(nb):
  p = planted_positions(nb)
  return sorted(set(p["batch_first"] + p["batch_last"] + p["last_piece"] + p["tail"]))


def dense_row(pattern, nb, k, q):
  """One row of scores, float32 [nb].  Rows of a call differ in pattern and in ``q``."""
  j = np.arange(nb, dtype=np.int64)
  if pattern == "equal":                          # the first k columns win
    return np.full(nb, 2.5, np.float32)
  if pattern == "ascending":                      # every offer passes: the maximum number of absorbs
    return ((j - 3000 + q) * 0.25).astype(np.float32)
  if pattern == "descending":                     # nothing passes once the first k are held
    return ((j - 3000 + q) * 0.25).astype(np.float32)[::-1].copy()
  if pattern == "tieblocks":                      # blocks of 48 ties: they straddle the 64-lane offers and column 2048
    return (((j // 48) * 7 + q) % 11 - 5).astype(np.float32)
  if pattern == "zeros":                          # +-0.0 mixed; a 1.0 every 97 columns
    v = np.array([-0.0, 0.0, -1.0, -0.0, 0.0, -2.0, -0.0], np.float32)[(j * 5 + q) % 7]
    v[(j % 97) == (q % 97)] = 1.0
    return v
  if pattern == "infs":                           # -inf every 13 columns, one +inf when it leaves room for a poison
    v = dense_row("tieblocks", nb, k, q)
    v[(j % 13) == 5] = -INF
    if k >= 2:
      v[(nb * 2) // 3] = INF
    return v
  assert pattern == "planted"                     # distinct winners at every seam over a floor of ties
  v = (-(1 + (j * 37) % 101)).astype(np.float32)
  at = np.array(all_planted(nb), np.int64)
  v[at] = 1000.0 + np.random.default_rng([nb, q]).permutation(at.size)
  return v


def row_pattern(q, shift=0):
  return PATTERNS[(q + shift) % len(PATTERNS)]


def dense_scores(nq, nb, k, shift=0):
  return np.stack([dense_row(row_pattern(q, shift), nb, k, q) for q in range(nq)])


def row_is_aligned(row, ld, offset):
  """Whether ``dense + row * ld`` is 16-byte aligned when the allocation is and ``dense`` lies ``offset`` floats in."""
  return (offset + row * ld) % 4 == 0


def dense_layouts(nb):
  """(ld, offset in floats) of every layout a row length runs in: rows packed, 1 .. 3 spare columns (rows then alternate
  between the two walks inside one launch whenever ld % 4 != 0), every row aligned, and a base pointer 4 bytes off."""
  ld4 = (nb + 3) & ~3
  return [(nb, 0), (nb + 1, 0), (nb + 2, 0), (nb + 3, 0), (ld4, 0), (ld4, 1)]


_DENSE = {}


def dense_case(nq, nb, k, state_len=0, shift=0, base_row=0, holes=False):
  """One ``tfrs_topk_update_from_scores`` call without its layout: ``scores`` [nq, nb]; the state ``state_bits`` /
  ``state_rows`` [nq, k] whose first ``state_len`` slots are a sorted list that ties with the new scores -- its rows
  lie above the block at ``base_row`` 0, below it at the top of the int32 range, on both sides in between -- and whose
  other slots are poisoned; with ``holes`` the last 1 .. 3 of the ``state_len`` slots carry row -1, as a paged search
  leaves them.  ``want_bits`` / ``want_rows`` is the list the call must leave, ``new_len`` what it must report."""
  key = (nq, nb, k, state_len, shift, base_row, holes)
  if key in _DENSE:
    return _DENSE[key]
  assert 0 <= state_len <= k <= MAX_K and base_row + nb <= TOP_ROW
  scores = dense_scores(nq, nb, k, shift)
  new_rows = base_row + np.arange(nb, dtype=np.int64)
  state_bits = np.full((nq, k), INF_BITS, np.uint32)                    # poison: beats every finite score
  state_rows = np.full((nq, k), POISON_ROW, np.int32)
  want_bits, want_rows = np.zeros((nq, k), np.uint32), np.full((nq, k), -1, np.int32)
  real = []
  for q in range(nq):
    n_holes = min(1 + q % 3, state_len) if holes else 0
    n_real = state_len - n_holes
    # an earlier block of n_real + 5 entries whose scores are this row's own finite ones (they tie with the new ones)
    i = np.arange(n_real + 5, dtype=np.int64)
    prev_s = np.resize(scores[q][::max(1, nb // (n_real + 5))], n_real + 5)
    prev_s[~np.isfinite(prev_s)] = 0.25
    below, above = base_row - 7 - 3 * i, base_row + nb + 100 + 3 * i
    prev_r = np.where(i % 2 == 0, below, above)
    prev_r = np.where(prev_r < 0, above, np.where(prev_r >= TOP_ROW, below, prev_r))
    assert prev_r.min() >= 0 and prev_r.max() < TOP_ROW and not np.intersect1d(prev_r, new_rows).size
    sb, sr = restated_topk(prev_s, prev_r, n_real)
    state_bits[q, :n_real], state_rows[q, :n_real] = sb, sr
    state_rows[q, n_real:state_len] = -1                                # holes keep a poison score: row -1 does not exist
    real.append((sb.view(np.float32), sr))
    want_bits[q], want_rows[q] = restated_topk(np.concatenate([sb.view(np.float32), scores[q]]),
                                               np.concatenate([sr.astype(np.int64), new_rows]), k)
  case = dict(nq=nq, nb=nb, k=k, state_len=state_len, base_row=base_row, scores=scores, state_bits=state_bits,
              state_rows=state_rows, want_bits=want_bits, want_rows=want_rows, new_len=min(k, state_len + nb),
              state_real=real, poison=INF)
  _DENSE[key] = case
  return case


FOLD_NB = 6151
FOLD_CUTS = ((0, 6151), (0, 2049, 6151), (0, 3, 67, 2115, 4167, 6151))      # 1, 2 and 5 consecutive calls


# ------------------------------------------------------------------------------------------ b. parts
MERGE_SHAPES = tuple((p, ki) for p in (1, 2, 8, 33) for ki in (1, 5, 100, 1024)) + (
    (1, 255), (1, 256), (1, 257), (1, 511), (2, 256), (1, 513), (1, 767), (3, 256), (1, 769))     # m around 256, 512, 768


def merge_k_outs(nparts, k_in):
  """k_out below, equal to and at the maximum allowed against nparts * k_in, and next to the KP switches in between."""
  m = nparts * k_in
  top = min(m, MAX_K)
  return sorted({1, top, min(m, 65), min(m, 129), max(1, top - 1), max(1, min(top, m // 2))})


_MERGE = {}


def merge_case(nparts, k_in, nq, few=False):
  """Parts [nparts, nq, k_in] of one merge: scores on a small alphabet with +-0.0 so that they tie across parts, rows
  interleaved over the parts (row = 7 + slot * nparts + part: equal scores meet with rows in every order), row -1 in
  scattered slots (their scores are poison) and, from two parts on, one part of every odd query that is all -1.  The last entry
  of the last part -- the one the walk re-reads at a clamped address -- holds the query's best score unless its part is
  the empty one.  ``few``: about one slot in a hundred exists (fewer than the larger k_out: empty slots) and query 0 has none."""
  key = (nparts, k_in, nq, few)
  if key in _MERGE:
    return _MERGE[key]
  rng = np.random.default_rng([nparts, k_in, nq, int(few)])
  alphabet = np.array([-0.0, 0.0, -1.5, 2.0, 2.0, 7.25, -3.0, 0.5], np.float32)
  scores = alphabet[rng.integers(0, alphabet.size, size=(nparts, nq, k_in))]
  p, q, j = np.meshgrid(np.arange(nparts), np.arange(nq), np.arange(k_in), indexing="ij")
  rows = (7 + j * nparts + p).astype(np.int64) + q * 11
  rows[:, 1::2] = 7 + ((k_in - 1 - j) * nparts + (nparts - 1 - p))[:, 1::2]     # odd queries: rows descend along a part
  scores[nparts - 1, :, k_in - 1] = 9.0
  gone = rng.random(size=rows.shape) < (0.99 if few else 0.15)
  gone[nparts - 1, :, k_in - 1] = False
  if few:
    gone[:, 0, :] = True                                      # query 0 of a `few` case has nothing at all
  empty_part = [(q_ + 1) % nparts if nparts >= 2 and (q_ % 2 == 1 or nq == 1) else -1 for q_ in range(nq)]
  for q_, ep in enumerate(empty_part):
    if ep >= 0:
      gone[ep, q_, :] = True
  rows[gone] = -1
  scores[gone] = INF                                                   # a slot that does not exist must not be read as one
  flat_s = scores.transpose(1, 0, 2).reshape(nq, -1)
  flat_r = rows.transpose(1, 0, 2).reshape(nq, -1)
  case = dict(nparts=nparts, k_in=k_in, nq=nq, scores=scores, rows=rows.astype(np.int32), flat_s=flat_s, flat_r=flat_r,
              empty_part=empty_part, poison=INF, poison_row=POISON_ROW)
  _MERGE[key] = case
  return case


def merge_want(case, k_out):
  out = [restated_topk(case["flat_s"][q], case["flat_r"][q], k_out) for q in range(case["nq"])]
  return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------------------------------ c. expand
EXPAND_K_IN = (1, 64, 65, 130)
EXPAND_K_OUT = (1, 5, 64, 65, 129, 300, 1024)


def duplicate_ranges(group_of_row):
  """(dup_start int64 [U + 1], dup_rows int32 [n], distinct_of_row) exactly as ``BruteForce.index`` builds them from
  the groups of bit-identical rows: distinct rows are numbered by ascending canonical (lowest) original row, and a
  distinct row's original rows are listed in ascending order (a stable sort of 0 .. n-1 by distinct row)."""
  group_of_row = np.asarray(group_of_row, np.int64)
  _, first, inverse = np.unique(group_of_row, return_index=True, return_inverse=True)
  rank = np.empty(first.size, np.int64)
  rank[np.argsort(first, kind="stable")] = np.arange(first.size)       # groups by ascending canonical row
  distinct_of_row = rank[inverse.reshape(-1)]
  dup_rows = np.argsort(distinct_of_row, kind="stable").astype(np.int32)
  dup_start = np.zeros(first.size + 1, np.int64)
  dup_start[1:] = np.cumsum(np.bincount(distinct_of_row, minlength=first.size))
  return dup_start, dup_rows, distinct_of_row


def expanded(case, q, upto=None):
  """(scores, original rows) of query q's results [0, upto) with every result replaced by all the rows it stands for."""
  s, u = case["scores"][q][:upto], case["distinct"][q][:upto]
  out_s, out_r = [], []
  for sc, uu in zip(s, u):
    if uu >= 0:
      r = case["dup_rows"][case["dup_start"][uu]:case["dup_start"][uu + 1]]
      out_r.append(r.astype(np.int64))
      out_s.append(np.full(r.size, sc, np.float32))
  if not out_s:
    return np.zeros(0, np.float32), np.zeros(0, np.int64)
  return np.concatenate(out_s), np.concatenate(out_r)


def expand_want(case, k_out):
  out = [restated_topk(*expanded(case, q), k_out) for q in range(case["nq"])]
  return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


_EXPAND = {}


def expand_case(k_in, k_out, nq, singles=False):
  """Results [nq, k_in] over a corpus whose distinct rows stand for 1, 2, 3, 63, 64, 65 and k_out + 3 original rows
  (``singles``: one each, the single-consume path), the original rows of a group scattered over the corpus.  Every query
  lists other distinct rows, in descending score order with ties (ties by ascending distinct row, as a search of the
  distinct index returns them), zeros of both signs, and row -1 in its last slots and, for odd queries, one slot in
  the middle."""
  key = (k_in, k_out, nq, singles)
  if key in _EXPAND:
    return _EXPAND[key]
  rng = np.random.default_rng([k_in, k_out, nq, int(singles)])
  n_distinct = k_in + 2 * nq + 9
  cycle = (1, 2, 1, 63, 1, 1, 64, 3, 1, 65, 1, k_out + 3, 1, 2, 1, 1)
  mult = np.ones(n_distinct, np.int64) if singles else np.array([cycle[(i * 5 + 1) % len(cycle)] for i in range(n_distinct)])
  group_of_row = rng.permutation(np.repeat(np.arange(n_distinct), mult))
  dup_start, dup_rows, distinct_of_row = duplicate_ranges(group_of_row)
  scores = np.zeros((nq, k_in), np.float32)
  distinct = np.full((nq, k_in), -1, np.int32)
  for q in range(nq):
    n_valid = max(1, k_in - q % 3) if k_in > 1 else 1 - (q == 3)
    u = np.sort(rng.permutation(n_distinct)[:n_valid])
    s = (2.0 - (np.arange(n_valid) // 3) * 0.5).astype(np.float32)      # runs of three equal scores, through +-0.0
    s[s == 0.0] = np.array([0.0, -0.0, 0.0], np.float32)[:int((s == 0.0).sum())]
    tied = restated_order(s, u)                                         # (score descending, distinct row ascending)
    scores[q, :n_valid], distinct[q, :n_valid] = s[tied], u[tied]
    if q % 2 == 1 and n_valid >= 4:
      distinct[q, n_valid // 2] = -1
      scores[q, n_valid // 2] = INF
    scores[q, n_valid:] = INF                                           # empty slots: poison scores
  case = dict(k_in=k_in, nq=nq, scores=scores, distinct=distinct, dup_start=dup_start, dup_rows=dup_rows,
              mult=np.diff(dup_start), distinct_of_row=distinct_of_row)
  _EXPAND[key] = case
  return case


EXPAND_TIE_K = (3, 4, 64, 66, 67, 130, 257)


def expand_tie_case(k_out, mode):
  """One query, k_out - 3 single results with higher scores, then result A (score s, original rows {lowest, high, high})
  and result B, which stands for two original rows BELOW A's high ones.  When B arrives the list holds exactly k_out
  entries and its last score is s.  ``mode`` "tie": B scores s as well and must displace A's two high rows (the early
  exit of the duplicate walk is strict); "lower": B scores less and changes nothing; "short": A stands for two rows
  only, so B arrives while k_out - 1 entries are held and its lower row enters."""
  n1 = k_out - 3
  # original rows: A = {0, 50 + n1, 51 + n1} (canonical 0), B = {1, 2} (canonical 1), the singles 3 .. n1 + 2, fillers
  group_of_row = np.full(60 + n1, -1, np.int64)
  a_rows = [0, 50 + n1, 51 + n1] if mode != "short" else [0, 50 + n1]
  group_of_row[a_rows] = 0
  group_of_row[[1, 2]] = 1
  rest = np.flatnonzero(group_of_row < 0)
  group_of_row[rest] = 2 + np.arange(rest.size)
  dup_start, dup_rows, distinct_of_row = duplicate_ranges(group_of_row)
  assert distinct_of_row[0] == 0 and distinct_of_row[1] == 1
  singles = distinct_of_row[3:3 + n1]
  s = np.float32(-0.0) if k_out % 2 else np.float32(1.0)                # (odd k_out: the tie is between zeros)
  sb = np.float32(0.0) if k_out % 2 else s
  scores = np.concatenate([np.full(n1, 5.0, np.float32), [s], [sb if mode != "lower" else np.float32(-1.0)],
                           [np.float32(-2.0)]]).astype(np.float32)[None]
  distinct = np.concatenate([singles, [0, 1], [distinct_of_row[40 + n1]]]).astype(np.int32)[None]
  return dict(k_in=n1 + 3, nq=1, scores=scores, distinct=distinct, dup_start=dup_start, dup_rows=dup_rows,
              mult=np.diff(dup_start), distinct_of_row=distinct_of_row, b_at=n1 + 1, mode=mode)


# ------------------------------------------------------------------------------------------ d. exclude
EXCLUDE_KIN = (1, 2, 63, 64, 65, 1029, 4096)
EXCLUDE_NE = (0, 1, 5)
EXCLUDE_ROWS = ("several", "absent", "all", "ties", "outranked")
PENALTY = np.float32(1.0e5)


def exclude_ks(kin):
  return sorted({1, max(1, kin - 1), kin, kin + 3})                     # k < kin, k == kin, k > kin


def exclude_restated(scores, ids, exclude, k):
  """The reference's arithmetic, literally, in float32: adjusted = score - 1e5 * isin, order (adjusted descending,
  column ascending), the ORIGINAL score bits and ids gathered.  Returns (bits uint32 [nq, kout], ids int32 [nq, kout],
  the order)."""
  nq, kin = scores.shape
  kout = min(k, kin)
  isin = (ids[:, :, None] == exclude[:, None, :]).any(axis=2) if exclude.shape[1] else np.zeros(ids.shape, bool)
  adjusted = (scores - PENALTY * isin.astype(np.float32)).astype(np.float32)
  order = np.stack([np.lexsort((np.arange(kin), -adjusted[q]))[:kout] for q in range(nq)])
  return (np.take_along_axis(bits(scores), order, 1), np.take_along_axis(ids, order, 1).astype(np.int32), order, isin)


_EXCLUDE = {}


def exclude_case(kin, ne):
  """scores / ids [5, kin] and exclude [5, ne], one row per entry of EXCLUDE_ROWS: an excluded id in several columns; an
  excluded id that occurs nowhere; every column excluded (the result is the original order); ties among the kept and
  among the excluded columns with zeros of both signs; and a kept score below (an excluded score - 1e5), so that the
  excluded column legitimately outranks it."""
  key = (kin, ne)
  if key in _EXCLUDE:
    return _EXCLUDE[key]
  rng = np.random.default_rng([kin, ne])
  nq = len(EXCLUDE_ROWS)
  c = np.arange(kin, dtype=np.int64)
  scores = rng.permutation(kin)[None].repeat(nq, 0).astype(np.float32) * 0.5 - 40.0
  ids = (100 + c * 3)[None].repeat(nq, 0).astype(np.int32)
  exclude = np.full((nq, ne), 99, np.int32)                             # 99 is nobody's id
  if ne:
    ids[0, c % 5 == 2] = 7                                              # "several": id 7 wherever column % 5 == 2
    exclude[0, ne - 1] = 7
    exclude[1, :] = np.arange(ne) * 3 + 101                             # "absent": between the ids, matches nothing
    ids[2] = 20 + c % ne                                                # "all": every id is excluded
    exclude[2] = 20 + np.arange(ne)
    ids[3] = 30 + c % 4                                                 # "ties": ids 30 and 32 excluded (ne 1: only 30)
    exclude[3, 0] = 30
    exclude[3, ne - 1] = 32 if ne > 1 else 30
    ids[4] = 50 + c % 3                                                 # "outranked": id 50 excluded
    exclude[4, ne // 2] = 50
  scores[3] = np.array([0.0, -0.0, 1.0, -0.0, 0.0, 1.0, -1.0], np.float32)[(c * 3) % 7]
  scores[4] = np.where(c % 3 == 0, 10.0, np.where(c % 3 == 1, -3.0e5, -4.0e4)).astype(np.float32)
  case = dict(kin=kin, ne=ne, nq=nq, scores=scores, ids=ids, exclude=exclude)
  _EXCLUDE[key] = case
  return case


# ------------------------------------------------------------------------------------------ the GPU entry points
def _lib():
  from recommenders_amd import _lib as L
  return L, L.load()


def _guarded(torch, nq, width, fill_bits=None, fill_rows=None):
  """int32 [nq + 2, width] of sentinels with rows 1 .. nq optionally filled; returns (buffer, view of the middle)."""
  buf = torch.full(((nq + 2) * width,), SENTINEL, dtype=torch.int32, device="cuda")
  mid = buf[width:(nq + 1) * width]
  src = fill_bits if fill_bits is not None else fill_rows
  if src is not None:
    mid.copy_(torch.from_numpy(np.ascontiguousarray(src).view(np.int32).reshape(-1)))
  return buf, mid


def _read(buf, nq, width):
  """(the middle rows as int32 [nq, width], whether both guard rows survived)."""
  a = buf.cpu().numpy()
  ok = bool((a[:width] == SENTINEL).all() and (a[(nq + 1) * width:] == SENTINEL).all())
  return a[width:(nq + 1) * width].reshape(nq, width), ok


def device_dense(scores, ld, offset, base_row, k, state_bits, state_rows, state_len, poison=INF, state=None):
  """One tfrs_topk_update_from_scores over ``scores`` [nq, nb] laid out with row stride ``ld``, ``offset`` floats into a
  16-byte aligned allocation whose every other float is ``poison``.  The state lies between guard rows.  ``state``:
  the (scores, rows) device buffers of an earlier call to update in place instead of a fresh state.  Returns
  (bits uint32 [nq, k], rows int32 [nq, k], new_len, guards intact, state buffers)."""
  import ctypes
  import torch
  L, lib = _lib()
  nq, nb = scores.shape
  assert ld >= nb and offset >= 0
  host = np.full(offset + nq * ld + 8, poison, np.float32)
  for q in range(nq):
    host[offset + q * ld: offset + q * ld + nb] = scores[q]
  buf = torch.from_numpy(host).cuda()
  assert buf.data_ptr() % 16 == 0
  if state is None:
    state = (_guarded(torch, nq, k, fill_bits=state_bits)[0], _guarded(torch, nq, k, fill_rows=state_rows)[0])
  st_s, st_r = state
  new_len = ctypes.c_int32(-7)
  L.check(lib.tfrs_topk_update_from_scores(
      ctypes.c_void_p(buf.data_ptr() + 4 * offset), nq, nb, ld, int(base_row), k, ctypes.c_void_p(st_s.data_ptr() + 4 * k),
      ctypes.c_void_p(st_r.data_ptr() + 4 * k), int(state_len), ctypes.byref(new_len), L.current_stream()))
  torch.cuda.synchronize()
  got_s, ok_s = _read(st_s, nq, k)
  got_r, ok_r = _read(st_r, nq, k)
  return got_s.view(np.uint32), got_r, new_len.value, ok_s and ok_r, state


def device_merge(case, k_out, stride=0):
  """tfrs_topk_merge (stride 0) or tfrs_topk_merge_strided with parts ``stride`` elements apart, the gaps poisoned
  (score above every real one, a valid row).  Returns (bits, rows, guards intact)."""
  import torch
  L, lib = _lib()
  nparts, nq, k_in = case["scores"].shape
  one = nq * k_in
  step = stride if stride else one
  assert step >= one
  hs = np.full(nparts * step + 8, case["poison"], np.float32)
  hr = np.full(nparts * step + 8, case["poison_row"], np.int32)
  for p in range(nparts):
    hs[p * step: p * step + one] = case["scores"][p].reshape(-1)
    hr[p * step: p * step + one] = case["rows"][p].reshape(-1)
  ts, tr = torch.from_numpy(hs).cuda(), torch.from_numpy(hr).cuda()
  out_s, out_r = _guarded(torch, nq, k_out)[0], _guarded(torch, nq, k_out)[0]
  po_s, po_r = L.c_void_p(out_s.data_ptr() + 4 * k_out), L.c_void_p(out_r.data_ptr() + 4 * k_out)
  if stride:
    L.check(lib.tfrs_topk_merge_strided(L.ptr(ts), L.ptr(tr), nparts, stride, nq, k_in, k_out, po_s, po_r,
                                        L.current_stream()))
  else:
    L.check(lib.tfrs_topk_merge(L.ptr(ts), L.ptr(tr), nparts, nq, k_in, k_out, po_s, po_r, None, 0, L.current_stream()))
  torch.cuda.synchronize()
  got_s, ok_s = _read(out_s, nq, k_out)
  got_r, ok_r = _read(out_r, nq, k_out)
  return got_s.view(np.uint32), got_r, ok_s and ok_r


def device_expand(case, k_out):
  """tfrs_topk_expand_duplicates; the result lists are followed by a poisoned row.  Returns (bits, rows, guards intact)."""
  import torch
  L, lib = _lib()
  nq, k_in = case["scores"].shape
  hs = np.concatenate([case["scores"].reshape(-1), np.full(k_in + 8, INF, np.float32)])
  hu = np.concatenate([case["distinct"].reshape(-1), np.zeros(k_in + 8, np.int32)])
  ts, tu = torch.from_numpy(hs).cuda(), torch.from_numpy(hu).cuda()
  tstart = torch.from_numpy(np.ascontiguousarray(case["dup_start"], np.int64)).cuda()
  trows = torch.from_numpy(np.ascontiguousarray(case["dup_rows"], np.int32)).cuda()
  out_s, out_r = _guarded(torch, nq, k_out)[0], _guarded(torch, nq, k_out)[0]
  L.check(lib.tfrs_topk_expand_duplicates(
      L.ptr(ts), L.ptr(tu), nq, k_in, L.ptr(tstart), L.ptr(trows), k_out, L.c_void_p(out_s.data_ptr() + 4 * k_out),
      L.c_void_p(out_r.data_ptr() + 4 * k_out), L.current_stream()))
  torch.cuda.synchronize()
  got_s, ok_s = _read(out_s, nq, k_out)
  got_r, ok_r = _read(out_r, nq, k_out)
  return got_s.view(np.uint32), got_r, ok_s and ok_r


def device_exclude(case, k):
  """tfrs_topk_exclude; returns (status, bits [nq, kout], ids [nq, kout], guards intact).  A refused call (status != 0)
  returns the status alone with the library's message."""
  import torch
  L, lib = _lib()
  nq, kin, ne = case["nq"], case["kin"], case["ne"]
  kout = min(k, kin)
  # one poisoned row before and after the inputs: ids that nobody excludes with winning scores
  hs = np.concatenate([np.full(kin, INF, np.float32), case["scores"].reshape(-1), np.full(kin, INF, np.float32)])
  hi = np.concatenate([np.zeros(kin, np.int32), case["ids"].reshape(-1), np.zeros(kin, np.int32)])
  ts, ti = torch.from_numpy(hs).cuda(), torch.from_numpy(hi).cuda()
  te = torch.from_numpy(np.ascontiguousarray(case["exclude"], np.int32).reshape(-1)).cuda() if ne else None
  out_s, out_i = _guarded(torch, nq, kout)[0], _guarded(torch, nq, kout)[0]
  rc = lib.tfrs_topk_exclude(L.c_void_p(ts.data_ptr() + 4 * kin), L.c_void_p(ti.data_ptr() + 4 * kin), nq, kin, L.ptr(te),
                             ne, k, L.c_void_p(out_s.data_ptr() + 4 * kout), L.c_void_p(out_i.data_ptr() + 4 * kout),
                             L.current_stream())
  if rc != 0:
    return rc, L.last_error(), None, None
  torch.cuda.synchronize()
  got_s, ok_s = _read(out_s, nq, kout)
  got_i, ok_i = _read(out_i, nq, kout)
  return rc, got_s.view(np.uint32), got_i, ok_s and ok_i
