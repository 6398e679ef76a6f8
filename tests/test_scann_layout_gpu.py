"""The ScaNN search kernels (csrc/scann.hip) on hand-built indexes (tests/scann_handbuilt.py) at the edges of the index
layout that a trained tree does not produce: leaves cut into several row ranges, several query tiles on such a leaf,
empty leaves that are probed, leaves of 1 / 127 / 128 / 129 rows, every k-step count of the scan, code rows up to the
64-byte ceiling with unused bytes, and every cell of the score buffer.  All comparisons are against the float64
restatement (tests/scann_restatement.py) under the bound of include/tfrs_hip.h, oracle.topk and BruteForce; nothing
here trains a tree."""

import numpy as np
import pytest

from oracle import topk as o_topk
from tests import scann_handbuilt as hb
from tests import scann_restatement as rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _ftk():
  from recommenders_amd.layers import factorized_top_k
  return factorized_top_k


def _np(x):
  return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _call(layer, q):
  s, rows = layer(q)
  return _np(s).copy(), _np(rows).copy()


# -- a. planted rows at every boundary --------------------------------------------------------------------------------
BOUNDARY_SIZES = [0, 1, 127, 128, 129, 4095, 4096, 4097, 9000, 0, 33]


@pytest.mark.parametrize("reorder", [None, 64])
def test_planted_rows_at_every_boundary(reorder, monkeypatch):
  """11 leaves (two empty, one of them first; 4095 / 4096 / 4097 / 9000 rows: one, one, two and three row ranges), all
  searched by 70 queries (three query tiles per leaf, the last of 6 pairs).  24 rows of each kind are planted next to
  the 32-row, 128-row and 4096-row boundaries of every leaf and at its last row; the restatement's band decides that a
  query's top 24 are exactly the planted rows of its kind (asserted on the host first), so a score that lands in another
  row's column changes the answer.  With re-ordering (R = 64 of 21 706 rows) the result is BruteForce's bit for bit.
  The same output with the queries in chunks of 33 and through a captured graph."""
  sizes = BOUNDARY_SIZES
  planted = hb.plant_edges(sizes)
  k = len(planted) // 2
  assert sorted(kind for _, kind in planted) == [14] * k + [15] * k
  off = np.concatenate([[0], np.cumsum(sizes)])
  for leaf, size in enumerate(sizes):      # both kinds in every leaf that can hold both
    kinds = {kind for pos, kind in planted if off[leaf] <= pos < off[leaf + 1]}
    assert len(kinds) == min(2, size), leaf
  state, c = hb.build_state(sizes, 20, 2, 1, planted, rows=True)
  q, even = hb.queries(70, 20, 2, 2)
  l_eff, p_max, probe_idx, _ = rs.probes(state, q, k, len(sizes))
  assert (l_eff, p_max) == (11, 21706)
  want, s64_of = [], []
  for b in range(len(q)):                  # the guard: the inputs decide all k rows
    orig, s64, eps = rs.candidates(state, q[b], probe_idx[b])
    sure = rs.surely_in(s64, eps, k)
    assert int(sure.sum()) == k, (b, int(sure.sum()))
    kind = 15 if even[b] else 14
    assert set(orig[sure].tolist()) == set(state["perm"][[p for p, kd in planted if kd == kind]].tolist()), b
    want.append(set(orig[sure].tolist()))
    s64_of.append({int(r): (s64[j], eps[j]) for j, r in enumerate(orig) if sure[j]})

  layer = hb.make_layer(state, k, len(sizes), reorder)
  assert layer.probe_plan(k) == (l_eff, p_max)
  s, rows = _call(layer, q)
  assert s.shape == (70, k) and rows.shape == (70, k)
  for b in range(len(q)):
    assert set(rows[b].tolist()) == want[b], (b, sorted(want[b] - set(rows[b].tolist())))
    assert hb.ordered(s[b], rows[b]), b
    if reorder is None:
      for j, r in enumerate(rows[b].tolist()):
        ref, eps = s64_of[b][r]
        assert abs(float(s[b, j]) - ref) <= eps, (b, r, float(s[b, j]), ref, eps)
  if reorder is not None:
    bs, bi = _ftk().BruteForce(k=k).index(c)(q)
    np.testing.assert_array_equal(rows, _np(bi))
    np.testing.assert_array_equal(s, _np(bs))
    es, ei = o_topk.brute_force(q, c, k)
    np.testing.assert_array_equal(rows, ei)
    np.testing.assert_array_equal(s, es)

  # chunks of 33 queries: the tile boundaries move, the output does not
  from recommenders_amd import _lib
  from recommenders_amd.layers.factorized_top_k import scann as scann_module
  lib, search, chunks = _lib.load(), _lib.load().tfrs_scann_search, []

  def counted_search(queries, nq, *rest):
    chunks.append(nq)
    return search(queries, nq, *rest)

  with monkeypatch.context() as m:
    m.setattr(lib, "tfrs_scann_search", counted_search)
    m.setattr(scann_module, "_SCANN_SCORE_BUDGET_BYTES", 4 * p_max * 33)
    s2, rows2 = _call(layer, q)
  assert chunks == [33, 33, 4]
  np.testing.assert_array_equal(rows2, rows)
  np.testing.assert_array_equal(s2, s)

  graphed = layer.make_graphed_call(q)
  for _ in range(3):
    s3, rows3 = graphed(q)
    np.testing.assert_array_equal(_np(rows3), rows)
    np.testing.assert_array_equal(_np(s3), s)


# -- b. every cell of the score buffer --------------------------------------------------------------------------------
_SPARSE = np.random.default_rng(1030).integers(0, 2, size=1030).tolist()    # 1030 leaves of 0 or 1 rows
CELL_SIZES = {"one1024": [1024], "ones40": [1] * 40, "gaps": [0, 0, 5, 0, 1000, 0], "full8": [128] * 8,
              "mixed": [127, 129, 1, 0, 255, 512], "sparse1030": _SPARSE}
CELL_DIMS = [(1, 1), (16, 1), (17, 2), (33, 2), (48, 3), (65, 2), (80, 1), (96, 4), (113, 7), (128, 1), (128, 2)]
CELL_NQ = [1, 33, 70]


def _cell_cases():
  """Paired, not crossed: every (d, dims_per_block) with three of the six size lists, nq and the garbage / wider code
  row alternating; then every size list once more at (20, 2) with 70 queries, and the 1030 sparse leaves at the
  64-byte code row."""
  names = list(CELL_SIZES)
  cases = []
  for i, (d, dpb) in enumerate(CELL_DIMS):
    for j in range(3):
      cases.append((names[(i + 2 * j) % 6], d, dpb, CELL_NQ[(i + j) % 3], (i + j) % 2 == 1))
  cases += [(name, 20, 2, 70, True) for name in names]
  cases.append(("sparse1030", 128, 1, 33, True))
  return cases


@pytest.mark.parametrize("name,d,dpb,nq,garbage", _cell_cases(),
                         ids=lambda v: str(v) if not isinstance(v, bool) else ("garbage" if v else "plain"))
def test_every_cell_of_the_score_buffer(name, d, dpb, nq, garbage):
  """At most 1024 rows, every leaf searched, no re-ordering, k = n: the call returns every row, so every score the
  scan wrote is compared with the float64 restatement.  The scan's k-step counts 1..8 (d = 1..128), odd and even block
  counts, the 64-byte code row of (128, 1); with ``garbage`` the unused nibble and bytes of a code row are random and
  the row is 4 bytes wider than needed where 64 allows."""
  sizes = CELL_SIZES[name]
  n = int(np.sum(sizes))
  nb = (d + min(dpb, d) - 1) // min(dpb, d)
  code_bytes = None
  if garbage and hb.min_code_bytes(nb) + 4 <= 64:
    code_bytes = hb.min_code_bytes(nb) + 4
  seed = 1000 * d + 10 * dpb + nq
  state = hb.build_state(sizes, d, dpb, seed, code_bytes=code_bytes, garbage=garbage)
  q, _ = hb.queries(nq, d, dpb, seed + 1)
  l_eff, p_max, probe_idx, _ = rs.probes(state, q, n, len(sizes))
  assert (l_eff, p_max) == (len(sizes), n)
  layer = hb.make_layer(state, n, len(sizes))
  s, rows = _call(layer, q)
  assert s.shape == (nq, n) and rows.shape == (nq, n)
  for b in range(nq):
    orig, s64, eps = rs.candidates(state, q[b], probe_idx[b])
    assert sorted(rows[b].tolist()) == list(range(n)), b
    ref, band = np.empty(n), np.empty(n)
    ref[orig], band[orig] = s64, eps
    err = np.abs(s[b].astype(np.float64) - ref[rows[b]])
    bad = err > band[rows[b]]
    assert not bad.any(), (b, rows[b][bad][:8].tolist(), float((err / band[rows[b]]).max()))
    assert hb.ordered(s[b], rows[b]), b


# -- c. partial probing with uneven leaves ----------------------------------------------------------------------------
PARTIAL_SIZES = [5000, 0, 3, 4097, 1, 128, 9000, 64]
PARTIAL_SEED = 2     # of three builder seeds tried on the host the one with the most distinct probe sets


@pytest.mark.parametrize("reorder", [None, 200])
def test_partial_probing_with_uneven_leaves(reorder):
  """3 of 8 leaves asked for, but the three smallest hold 4 rows: the planner widens to 4 leaves (18 225 columns).  200
  queries probe many different leaf sets, with multi-range leaves, an empty leaf and a 1-row leaf among them; the
  assertions are those of test_kernels_against_restatement.  Two conditions on the inputs, evaluated on the host
  first, keep it from passing on nothing: at least 8 distinct probe sets, and on average at least 0.8 of the k rows
  decided by the band."""
  k, nls = 10, 3
  planted = hb.plant_edges(PARTIAL_SIZES)
  state, c = hb.build_state(PARTIAL_SIZES, 20, 2, PARTIAL_SEED, planted, rows=True)
  q, _ = hb.queries(200, 20, 2, 100 + PARTIAL_SEED)
  assert rs.probe_width(PARTIAL_SIZES, nls, k) == (4, 18225)
  distinct, share = hb.decided_share(state, q, k, nls)
  print("distinct probe sets", distinct, "mean decided share", share)
  assert distinct >= 8, distinct
  assert share >= 0.8, share
  layer = hb.make_layer(state, k, nls, reorder)
  assert layer.probe_plan(10) == (4, 18225)
  s, rows = _call(layer, q)
  hb.check_against_restatement(layer, state, q, k, nls, reorder, s, rows, corpus=c)


# -- d. degenerate queries --------------------------------------------------------------------------------------------
DEGENERATE_SIZES = CELL_SIZES["mixed"]       # 1024 rows, an empty leaf


def _degenerate_index(planted=()):
  return hb.build_state(DEGENERATE_SIZES, 48, 3, 77, planted, rows=True)


def test_zero_query_and_identical_rows_equal_bruteforce():
  """An all-zero query, and 300 bit-identical rows (one leaf, one code) that tie at the top of half the queries: ScaNN
  with every row re-ordered is BruteForce bit for bit, ties to the lower original row."""
  off = np.concatenate([[0], np.cumsum(DEGENERATE_SIZES)])
  planted = [(int(off[5]) + 7 + r, 15) for r in range(300)]
  state, c = _degenerate_index(planted)
  assert len(np.unique(state["rows"][[p for p, _ in planted]], axis=0)) == 1
  q, even = hb.queries(40, 48, 3, 78)
  assert 5 <= int(even.sum()) <= 35
  q[3] = 0.0
  k = 50
  layer = hb.make_layer(state, k, len(DEGENERATE_SIZES), 1024)
  s, rows = _call(layer, q)
  bs, bi = _ftk().BruteForce(k=k).index(c)(q)
  np.testing.assert_array_equal(rows, _np(bi))
  np.testing.assert_array_equal(s, _np(bs))
  es, ei = o_topk.brute_force(q, c, k)
  np.testing.assert_array_equal(rows, ei)
  np.testing.assert_array_equal(s, es)
  assert rows[3].tolist() == list(range(k)) and not s[3].any()
  tied = sorted(state["perm"][[p for p, _ in planted]].tolist())
  for b in np.flatnonzero(even):
    if b != 3:
      assert rows[b].tolist() == tied[:k], b


@pytest.mark.parametrize("exponent", [-60, 60])
def test_query_scale(exponent):
  """Queries times 2^-60 and 2^+60 (every product stays a normal f32): the same rows, and the re-ordered scores are
  exactly the unscaled ones times that power of two."""
  state, c = _degenerate_index()
  q, _ = hb.queries(70, 48, 3, 79)
  layer = hb.make_layer(state, 20, len(DEGENERATE_SIZES), 1024)
  s1, rows1 = _call(layer, q)
  s2, rows2 = _call(layer, q * np.float32(2.0 ** exponent))
  np.testing.assert_array_equal(rows2, rows1)
  np.testing.assert_array_equal(s2, s1 * np.float32(2.0 ** exponent))


@pytest.mark.parametrize("reorder", [None, 1024])
def test_nan_and_inf_queries_do_not_leak(reorder):
  """Query 7 holds a NaN and query 40 an Inf: every other query's output is bit-identical to the batch without them
  (a query is one column of the MFMA tile; it must not reach its tile neighbours).  The two bad queries themselves
  are outside the contract: only the shape of their output is fixed."""
  state, c = _degenerate_index()
  q, _ = hb.queries(70, 48, 3, 80)
  layer = hb.make_layer(state, 20, len(DEGENERATE_SIZES), reorder)
  s1, rows1 = _call(layer, q)
  bad = q.copy()
  bad[7, 5] = np.nan
  bad[40, 11] = np.inf
  s2, rows2 = _call(layer, bad)
  assert s2.shape == (70, 20) and rows2.shape == (70, 20)
  keep = np.setdiff1d(np.arange(70), [7, 40])
  np.testing.assert_array_equal(rows2[keep], rows1[keep])
  np.testing.assert_array_equal(s2[keep], s1[keep])
