"""Hand-built corpora for the rank-count metric kernels (csrc/metric_fused.hip: ``rank_count_kernel<DP>``,
``hits_update_kernel``): every builder returns the three matrices of one ``tfrs_rank_count_accumulate`` call together
with what it planted -- for every query the exact number of candidates that beat its positive -- so a test compares
the ``counts`` buffer itself, query by query, instead of a mean of hits that one dropped or double-counted candidate
position does not move.  The launch planner is restated here, with helpers that list the candidate positions at every
edge of a launch geometry (tile boundaries, split starts, the ragged last tile);
tests/test_metric_handbuilt_host.py proves every planted property again from the arrays alone, in float64, and the
restated geometry against the library's own ``tfrs_rank_count_plan``.  Pure numpy at import; ``device_counts`` and
``device_hits_update`` (the functions that touch the GPU) import torch when they are called.  Test infrastructure only.

Every builder keeps to integers, half-integers or multiples of 1/16 far below 2^23, so every product and every partial
sum of a score is exact in float32 in any summation order: the device decides ``score > positive`` exactly as float64
does, and the comparison is ``array_equal`` on integers."""

import numpy as np

TILE = 32
QTILE = 128
NONFINITE_BIT = 0x80000000
COUNT_MASK = 0x7FFFFFFF
WIDTHS = (0, 1, 2, 33)
MAX_WINDOW_ROWS = 2890         # (nc - 1)^2 < 2^23: -j^2 and every score stay exact in float32


# ------------------------------------------------------------------------------------------ the planner, restated
def padded_dim(d):
  for dp in (8, 16, 32, 64):
    if d <= dp:
      return dp
  return 128


def plan(nq, nc, d):
  """[n_qtiles, tiles_per_split, nsplits, max_tiles] of tfrs_rank_count_accumulate at (nq, nc, d)."""
  n_qtiles = (nq + QTILE - 1) // QTILE
  max_tiles = 7 if padded_dim(d) <= 64 else 3
  ntiles = (nc + TILE - 1) // TILE
  want = max(1, 256 // n_qtiles)
  tps = min(max_tiles, max(1, (ntiles + want - 1) // want))
  return [n_qtiles, tps, (ntiles + tps - 1) // tps, max_tiles]


def split_shape(nq, nc, d):
  """(tiles per split, number of splits, tiles of the last split, rows of the last tile)."""
  _, tps, nsplits, _ = plan(nq, nc, d)
  ntiles = (nc + TILE - 1) // TILE
  return tps, nsplits, ntiles - (nsplits - 1) * tps, nc - (ntiles - 1) * TILE


def edge_positions(nq, nc, d):
  """Candidate positions at every edge of the launch geometry, ascending: 0 and nc - 1, the rows on both sides of
  every tile boundary, every split start and its predecessor, and every row of the last tile."""
  _, tps, nsplits, _ = plan(nq, nc, d)
  ntiles = (nc + TILE - 1) // TILE
  pos = {0, nc - 1}
  for t in range(1, ntiles):
    pos.update((TILE * t - 1, TILE * t, TILE * t + 1))
  for s in range(1, nsplits):
    pos.update((TILE * tps * s - 1, TILE * tps * s))
  pos.update(range(TILE * (ntiles - 1), nc))
  return sorted(p for p in pos if 0 <= p < nc)


# ------------------------------------------------------------------------------------------ the plain reference
def reference_counts(q, true_c, cand, chunk=2048):
  """(counts int64 [nq], nonfinite bool [nq]): float64 scores, the float64 positive, the number of candidates whose
  score is STRICTLY greater, and whether the positive's score is not finite.  Shares nothing with the kernel."""
  q64, t64, c64 = (np.asarray(x, np.float64) for x in (q, true_c, cand))
  with np.errstate(invalid="ignore", over="ignore"):
    pos = (q64 * t64).sum(axis=1)
    counts = np.zeros(q64.shape[0], np.int64)
    for lo in range(0, q64.shape[0], chunk):
      s = q64[lo:lo + chunk] @ c64.T
      counts[lo:lo + chunk] = (s > pos[lo:lo + chunk, None]).sum(axis=1)
  return counts, ~np.isfinite(pos)


# ------------------------------------------------------------------------------------------ builders
def live_pairs(d):
  """Placements (k0, k1) of the two live coordinates of ``windows``: the first and the last feature, and an odd / even
  pair that straddles a 4-float chunk (d >= 5; below that the first pair the other way round).  Empty at d = 1: the
  construction needs two coordinates."""
  if d < 2:
    return ()
  if d < 5:
    return ((0, d - 1), (d - 1, 0))
  chunk = ((d - 5) // 4) // 2             # a middle chunk boundary: features 4 chunk + 3 | 4 chunk + 4
  return ((0, d - 1), (4 * chunk + 3, 4 * chunk + 4))


def window_plan(rng, nq, nc, d):
  """(centres, widths) of ``windows``: every edge position of the geometry as a centre with every width, width 1 first
  (that window is the edge position alone), then 2, 33 and 0, as far as ``nq`` goes; the remaining queries are random."""
  edges = edge_positions(nq, nc, d)
  pairs = [(e, w) for w in (1, 2, 33, 0) for e in edges][:nq]
  centres = np.array([p[0] for p in pairs], np.int64)
  widths = np.array([p[1] for p in pairs], np.int64)
  rest = nq - len(pairs)
  centres = np.concatenate([centres, rng.integers(0, nc, size=rest)])
  widths = np.concatenate([widths, rng.choice(np.array(WIDTHS), size=rest)])
  return centres, widths


def windows(nq, nc, d, k0, k1, centres, widths, tie):
  """Candidate j holds 2 j at k0 and -j^2 at k1, query b holds centre_b at k0 and 1 at k1, so
  score(b, j) = centre_b^2 - (j - centre_b)^2; the positive row holds centre_b^2 - width_b^2 (+ 0.5 unless ``tie``)
  at k1.  The candidates that beat the positive are exactly those with |j - centre_b| < width_b (none at width 0);
  with ``tie`` the two candidates at distance width_b equal the positive exactly and must not count.  ``counts`` is
  that window clipped to [0, nc), in closed form.  The canary row beats every positive."""
  assert 1 <= nc <= MAX_WINDOW_ROWS, nc
  assert k0 != k1 and 0 <= k0 < d and 0 <= k1 < d
  centres, widths = np.asarray(centres, np.int64), np.asarray(widths, np.int64)
  assert centres.shape == widths.shape == (nq,) and centres.min() >= 0 and centres.max() < nc
  j = np.arange(nc, dtype=np.int64)
  cand = np.zeros((nc, d), np.float32)
  cand[:, k0] = 2 * j
  cand[:, k1] = -(j * j)
  q = np.zeros((nq, d), np.float32)
  q[:, k0] = centres
  q[:, k1] = 1.0
  true_c = np.zeros((nq, d), np.float32)
  true_c[:, k1] = centres * centres - widths * widths + (0.0 if tie else 0.5)
  lo, hi = np.maximum(centres - widths + 1, 0), np.minimum(centres + widths - 1, nc - 1)
  counts = np.where(widths > 0, np.maximum(hi - lo + 1, 0), 0)
  canary = np.zeros(d, np.float32)
  canary[k1] = 2.0 ** 23                   # score 2^23 for every query: above every centre^2 + 0.5
  harmless = np.zeros(d, np.float32)
  harmless[k1] = -(2.0 ** 23)              # ... and a row that beats no positive
  return dict(kind="windows", q=q, true_c=true_c, cand=cand, counts=counts, canary=canary, harmless=harmless,
              centres=centres, widths=widths, k0=k0, k1=k1, tie=tie)


def grid(rng, nq, nc, d):
  """All three matrices on {-3 .. 3} / 4 in every coordinate (coordinate d // 2 of the queries on {1, 2, 3} / 4: what
  the canary row needs), every third positive an exact copy of a corpus row -- it ties with its copy, which must not
  count.  Every feature takes part in every score: a coordinate paired with the wrong partner changes the counts."""
  cand = (rng.integers(-3, 4, size=(nc, d)) / 4.0).astype(np.float32)
  q = (rng.integers(-3, 4, size=(nq, d)) / 4.0).astype(np.float32)
  kc = d // 2
  q[:, kc] = rng.integers(1, 4, size=nq) / 4.0
  true_c = (rng.integers(-3, 4, size=(nq, d)) / 4.0).astype(np.float32)
  copies = np.arange(0, nq, 3)
  copied_rows = rng.integers(0, nc, size=copies.size)
  copied_rows[:min(copies.size, 2)] = (0, nc - 1)[:min(copies.size, 2)]
  true_c[copies] = cand[copied_rows]
  canary = np.zeros(d, np.float32)
  canary[kc] = 4.0 * (d * 9.0 / 16.0 + 1.0)          # score >= d 9/16 + 1 > every |positive|
  harmless = -canary
  return dict(kind="grid", q=q, true_c=true_c, cand=cand, counts=None, canary=canary, harmless=harmless,
              copies=copies, copied_rows=copied_rows)


def with_ids(case, vocab, id_dtype, rng):
  """The case's candidate rows scattered into a ``vocab``-row table through a permutation; every table row that no id
  names is a canary.  Some ids are duplicated (the row they named becomes a canary), some are out of range and must
  score as zero rows: -1, ``vocab`` and, for int64 ids, 2^32 + (a canary's row).  ``cand`` is what the ids say, row by
  row; ``negative`` marks the positives below 0, which every zero row beats."""
  cand = case["cand"]
  nc, d = cand.shape
  assert vocab > nc
  perm = rng.permutation(vocab)
  ids = perm[:nc].astype(np.int64)
  spare = int(perm[nc])                                # a row no id names
  # (what, position), first come first served on distinct positions: small corpora take what fits
  wanted = [("negative", nc - 1), ("vocab", 0), ("dup", nc // 3), ("dup", TILE if nc > TILE + 1 else 1)]
  if np.dtype(id_dtype) == np.int64:
    wanted.insert(2, ("wide", nc // 2))
  taken, mods = set(), []
  for what, at in wanted:
    src = at + 1                                       # a duplicate names the row of its right neighbour
    if at in taken or not 0 <= at < nc or (what == "dup" and (src >= nc or src in taken)):
      continue
    taken.update((at, src) if what == "dup" else (at,))
    mods.append((what, at))
    ids[at] = ids[src] if what == "dup" else {"negative": -1, "vocab": vocab, "wide": 2 ** 32 + spare}[what]
  ids = ids.astype(id_dtype)
  # the table, in the order of the writes: all canaries; then candidate j into row perm[j] for every j; then canaries
  # again over every row that no valid id names any more (the rows a duplicate or an out-of-range id stopped naming)
  valid = (ids >= 0) & (ids < vocab)
  table = np.tile(case["canary"], (vocab, 1)).astype(np.float32)
  table[perm[:nc]] = cand
  unnamed = np.setdiff1d(np.arange(vocab), ids[valid].astype(np.int64))
  table[unnamed] = case["canary"]
  eff = np.where(valid[:, None], table[np.clip(ids.astype(np.int64), 0, vocab - 1)], 0.0).astype(np.float32)
  pos = (case["q"].astype(np.float64) * case["true_c"].astype(np.float64)).sum(axis=1)
  out = dict(case, cand=eff, table=table, ids=ids, vocab=vocab, mods=mods, zero_rows=np.flatnonzero(~valid),
             negative=pos < 0, spare=spare, unnamed=unnamed, base=case)
  for stale in ("counts", "ref", "ref_nonfinite"):      # the base's: with_reference computes the scattered case's own
    out.pop(stale, None)
  return out


def with_canary_tail(case, extra):
  """The candidate block as the prefix of a larger allocation whose rows past nc hold canaries; nc is still the row
  count handed to the kernel."""
  alloc = np.concatenate([case["cand"], np.tile(case["canary"], (extra, 1))]).astype(np.float32)
  return dict(case, alloc=alloc)


def inbatch_windows(nq, nc, d, k0, k1, rng):
  """The ``windows`` corpus seen by ``TopKCategoricalAccuracy.update_from_embeddings`` (labels = eye: the positive of
  query b is candidate b).  Query b centres on b + width_b or b - width_b, so the candidates that beat its positive are
  those with |j - centre_b| < width_b; candidate b itself and its mirror tie and do not count."""
  assert nq <= nc
  widths = rng.choice(np.array(WIDTHS), size=nq)
  sign = rng.choice(np.array([-1, 1]), size=nq)
  centres = np.arange(nq) + sign * widths
  centres = np.where((centres < 0) | (centres >= nc), np.arange(nq) - sign * widths, centres)
  centres = np.where((centres < 0) | (centres >= nc), np.arange(nq), centres)
  widths = np.abs(centres - np.arange(nq))
  case = windows(nq, nc, d, k0, k1, centres, widths, tie=True)      # (its positive row scores what candidate b scores)
  return case["q"], case["cand"], case["counts"]


# ------------------------------------------------------------------------------------------ the cases, shared by both tests
# (nq, nc) -> dims, and what the launch reaches: (tiles per split, splits, tiles of the last split, rows of the last tile)
GEOMETRIES = (
    ((1, 1), (1, 4), (1, 1, 1, 1)),
    ((33, 40), (1, 4), (1, 2, 1, 8)),
    ((130, 229), (7,), (1, 8, 1, 5)),
    ((4700, 1381), (8, 20, 64), (7, 7, 2, 5)),
    ((16400, 450), (16,), (7, 3, 1, 2)),
    ((8300, 293), (100, 128), (3, 4, 1, 5)),
    ((8300, 2890), (32,), (7, 13, 7, 10)),
)
# every tiles-per-split between the two ends: one query tile more than 128 leaves one split per tile count
DEPTH_SHAPES = {(16400, 40, 8): 2, (16400, 70, 8): 3, (16400, 100, 16): 4, (16400, 131, 8): 5, (16400, 161, 8): 6,
                (16400, 40, 128): 2}
DIM_SWEEP_SHAPE = (130, 229)
DIM_SWEEP = (1, 2, 3, 4, 5, 9, 12, 17, 31, 33, 60, 65, 127)
QUERY_EDGE_NQ = (1, 31, 32, 33, 127, 128, 129)
QUERY_EDGE_NC, QUERY_EDGE_D = 229, 12
ID_GEOMETRIES = tuple((nq, nc, d) for (nq, nc), dims, _ in GEOMETRIES for d in dims if padded_dim(d) <= 32) + (
    (8300, 293, 100),)
BLOCK_ROWS = (1, 31, 32, 33, 229, 7, 224, 64, 450)      # a 1071-row corpus in blocks
NONFINITE_SHAPES = ((700, 229, 12), (8300, 2890, 32))   # an even (8) and an odd (13) number of splits


def layout_cases():
  """(nq, nc, d) of every counts case of tests/test_metric_layout_gpu.py, in order, without repeats."""
  out = [(nq, nc, d) for (nq, nc), dims, _ in GEOMETRIES for d in dims]
  out += list(DEPTH_SHAPES)
  out += [DIM_SWEEP_SHAPE + (d,) for d in DIM_SWEEP]
  out += [(nq, QUERY_EDGE_NC, QUERY_EDGE_D) for nq in QUERY_EDGE_NQ]
  return list(dict.fromkeys(out))


def case_rng(tag, nq, nc, d):
  return np.random.default_rng([sum(map(ord, tag)), nq, nc, d])


_CASES = {}


def build(family, nq, nc, d, pair=0):
  """The case of ``family`` ("windows", "windows_tie", "grid") at a shape, built once and shared; every case carries its
  reference counts (``ref``) and flags (``ref_nonfinite``)."""
  key = (family, nq, nc, d, pair)
  if key not in _CASES:
    rng = case_rng(family, nq, nc, d)
    if family == "grid":
      case = grid(rng, nq, nc, d)
    else:
      k0, k1 = live_pairs(d)[pair]
      centres, widths = window_plan(rng, nq, nc, d)
      case = windows(nq, nc, d, k0, k1, centres, widths, tie=family == "windows_tie")
    _CASES[key] = with_reference(case)
  return _CASES[key]


def with_reference(case):
  case = dict(case)
  case["ref"], case["ref_nonfinite"] = reference_counts(case["q"], case["true_c"], case["cand"])
  return case


def families(d):
  """(family, pair) of every case a geometry runs: both placements of ``windows`` with and without ties, and ``grid``."""
  out = [(f, p) for p in range(len(live_pairs(d))) for f in ("windows", "windows_tie")]
  return out + [("grid", 0)]


# ------------------------------------------------------------------------------------------ the hits kernel's inputs
HITS_KS = {1: (7,), 5: (10, 1, 2 ** 31 - 1, 21, 5),
           16: (10, 1, 21, 2 ** 31 - 1, 5, 2, 20, 3, 19, 4, 18, 6, 17, 8, 11, 15)}
HITS_NQ = (1, 1023, 1025, 16384, 16385, 20000)


def hits_inputs(nq, weighted):
  """(counts uint32 with some bit-31 flags, weights float32 or None): counts 0 .. 20, every fifth flagged not finite,
  weights on multiples of 1/4 with zeros."""
  b = np.arange(nq, dtype=np.int64)
  counts = ((b * 7 + b // 21) % 21).astype(np.uint32)
  counts[b % 5 == 3] |= np.uint32(NONFINITE_BIT)
  w = (((b * 3 + b // 9) % 9) / 4.0).astype(np.float32) if weighted else None
  return counts, w


def hits_reference(counts, ks, w):
  """(hits float64 [nks, nq], state float64 [2 nks]) of one tfrs_topk_hits_update from zero state."""
  counts = np.asarray(counts, np.uint32)
  finite = (counts & np.uint32(NONFINITE_BIT)) == 0
  low = (counts & np.uint32(COUNT_MASK)).astype(np.int64)
  hits = np.stack([(finite & (low < int(k))).astype(np.float64) for k in ks])
  w64 = np.ones(counts.shape[0]) if w is None else np.asarray(w, np.float64)
  return hits, np.concatenate([hits @ w64, np.full(len(ks), w64.sum())])


# ------------------------------------------------------------------------------------------ the GPU entry points
def device_counts(q, true_c, cand, nc=None, ids=None, vocab=None, first_block=1, counts=None):
  """The raw uint32 ``counts`` buffer after one tfrs_rank_count_accumulate (read before any re-arm).  ``cand`` is the
  candidate block, or the table when ``ids`` is given; ``counts``: a device buffer to add into (returned as well)."""
  import torch
  from recommenders_amd import _lib
  lib = _lib.load()
  tq, tt = (torch.as_tensor(np.ascontiguousarray(x, np.float32)).cuda() for x in (q, true_c))
  tc = cand if isinstance(cand, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(cand, np.float32)).cuda()
  nq, d = tq.shape
  assert tt.shape == tq.shape and tc.shape[1] == d and tc.is_contiguous()
  tids = None
  if ids is not None:
    assert ids.dtype in (np.int32, np.int64)
    tids = torch.as_tensor(np.ascontiguousarray(ids)).cuda()
    nc = ids.shape[0] if nc is None else nc
    assert nc <= ids.shape[0]
  nc = tc.shape[0] if nc is None else nc
  vocab = tc.shape[0] if vocab is None else vocab
  assert vocab <= tc.shape[0] and (ids is not None or nc <= tc.shape[0])      # nothing is read past an allocation
  if counts is None:
    counts = torch.zeros((nq,), dtype=torch.int32, device=tq.device)
  assert counts.shape == (nq,) and counts.dtype == torch.int32
  _lib.check(lib.tfrs_rank_count_accumulate(
      _lib.ptr(tq), _lib.ptr(tt), nq, d, _lib.ptr(tc), _lib.ptr(tids), 1 if ids is not None and ids.dtype == np.int64 else 0,
      nc, vocab, _lib.ptr(counts), int(first_block), _lib.current_stream()))
  return counts.cpu().numpy().view(np.uint32), counts


def device_hits_update(counts, ks, w, state=None, want_hits=True):
  """(hits [nks, nq] or None, state [2 nks], results [nks], counts afterwards) of one tfrs_topk_hits_update on a uint32
  ``counts`` array; ``state``: the float32 state of an earlier call to add to."""
  import ctypes
  import torch
  from recommenders_amd import _lib
  lib = _lib.load()
  nq, nks = counts.shape[0], len(ks)
  tcnt = torch.as_tensor(np.ascontiguousarray(counts, np.uint32).view(np.int32)).cuda()
  tw = None if w is None else torch.as_tensor(np.ascontiguousarray(w, np.float32)).cuda()
  tstate = torch.zeros((2 * nks,), dtype=torch.float32, device=tcnt.device)
  if state is not None:
    tstate.copy_(torch.as_tensor(np.asarray(state, np.float32)))
  tres = torch.full((nks,), -1.0, dtype=torch.float32, device=tcnt.device)
  thits = torch.full((nks, nq), -1.0, dtype=torch.float32, device=tcnt.device) if want_hits else None
  ks_arr = (ctypes.c_int32 * nks)(*[int(k) for k in ks])
  _lib.check(lib.tfrs_topk_hits_update(_lib.ptr(tcnt), nq, ks_arr, nks, _lib.ptr(tw), _lib.ptr(tstate), _lib.ptr(tres),
                                       _lib.ptr(thits), _lib.current_stream()))
  return (None if thits is None else thits.cpu().numpy(), tstate.cpu().numpy(), tres.cpu().numpy(),
          tcnt.cpu().numpy().view(np.uint32))
