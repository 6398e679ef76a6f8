"""The hand-built corpora of tests/metric_handbuilt.py, proved on the host: every property a case of
tests/test_metric_layout_gpu.py relies on is derived again from the arrays alone, in float64, and the launch geometry
each case claims is asked from the library's own planner (``tfrs_rank_count_plan``, the function
``tfrs_rank_count_accumulate`` calls).  No GPU access: the plan entry point does no device work."""

import ctypes

import numpy as np
import pytest

from recommenders_amd import _lib
from tests import metric_handbuilt as hb

# every shape the GPU test uses; at the large ones the explicit float32 products run on one variant of ``windows``
# (test_windows_cases_plant_what_they_say says why), every other property on all of them
BIG_CASES = [s for s in hb.layout_cases() if s[0] * s[1] > 10 ** 6]
SMALL_CASES = [s for s in hb.layout_cases() if s not in BIG_CASES]


def lib_plan(nq, nc, d):
  out = (ctypes.c_int64 * 4)()
  _lib.check(_lib.load().tfrs_rank_count_plan(nq, nc, d, out))
  return list(out)


# ------------------------------------------------------------------------------------------ geometry
def test_plan_entry_point_rejects_bad_arguments():
  out = (ctypes.c_int64 * 4)()
  lib = _lib.load()
  assert lib.tfrs_rank_count_plan(0, 5, 8, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_rank_count_plan(5, 0, 8, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_rank_count_plan(5, 5, 0, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_rank_count_plan(5, 5, 129, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_rank_count_plan(5, 5, 8, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_rank_count_plan(5, 5, 128, out) == _lib.TFRS_OK and list(out) == [1, 1, 1, 3]


def test_restated_planner_equals_the_librarys_over_a_sweep():
  nqs = (1, 127, 128, 129, 700, 4096, 4700, 8300, 10880, 10881, 16384, 16385, 32768, 32769, 100000)
  ncs = (1, 31, 32, 33, 229, 293, 450, 1381, 1682, 2890, 50000, 1000003)
  seen = set()
  for nq in nqs:
    for nc in ncs:
      for d in (1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128):
        got = lib_plan(nq, nc, d)
        assert got == hb.plan(nq, nc, d), (nq, nc, d)
        ntiles = (nc + 31) // 32
        assert 1 <= got[1] <= got[3] and (got[2] - 1) * got[1] < ntiles <= got[2] * got[1]      # no empty split
        seen.add((got[3], got[1]))
  assert {t for m, t in seen if m == 7} == set(range(1, 8)) and {t for m, t in seen if m == 3} == {1, 2, 3}


@pytest.mark.parametrize("shape,dims,claimed", hb.GEOMETRIES, ids=lambda v: str(v).replace(" ", ""))
def test_geometries_reach_what_the_table_says(shape, dims, claimed):
  nq, nc = shape
  for d in dims:
    assert lib_plan(nq, nc, d) == hb.plan(nq, nc, d)
    assert hb.split_shape(nq, nc, d) == claimed, (d, hb.split_shape(nq, nc, d))


def test_geometry_table_details():
  assert [hb.padded_dim(d) for d in (1, 4, 7, 8, 20, 64, 16, 100, 128, 32)] == [8, 8, 8, 8, 32, 64, 16, 128, 128, 32]
  assert lib_plan(130, 229, 7)[0] == 2 and lib_plan(4700, 1381, 8)[0] == 37
  assert lib_plan(8300, 2890, 32)[1:3] == [7, 13] and 13 * 7 * 32 >= 2890 > (13 * 7 - 1) * 32
  for (nq, nc, d), tiles in hb.DEPTH_SHAPES.items():
    assert lib_plan(nq, nc, d)[1:3] == [tiles, 1] and nc % 32 != 0
  depths = {(hb.padded_dim(d) > 64, hb.plan(nq, nc, d)[1]) for nq, nc, d in hb.layout_cases()}
  assert depths == {(False, t) for t in range(1, 8)} | {(True, t) for t in (1, 2, 3)}      # every depth is reached
  assert {lib_plan(*s)[2] % 2 for s in hb.NONFINITE_SHAPES} == {0, 1}
  assert sum(hb.BLOCK_ROWS) == 1071 and {1, 31, 32, 33, 229} <= set(hb.BLOCK_ROWS)
  assert all(hb.padded_dim(d) <= 32 for _, _, d in hb.ID_GEOMETRIES[:-1]) and hb.padded_dim(hb.ID_GEOMETRIES[-1][2]) == 128
  assert {d % 4 == 0 for d in hb.DIM_SWEEP} == {True, False} and any(d < hb.padded_dim(d) for d in hb.DIM_SWEEP)


def test_edge_positions():
  assert hb.edge_positions(1, 1, 8) == [0]
  assert hb.edge_positions(33, 40, 4) == [0, 31, 32, 33, 34, 35, 36, 37, 38, 39]
  e = hb.edge_positions(4700, 1381, 20)                   # 7 tiles per split: split starts at multiples of 224
  assert {0, 1380, 223, 224, 1343, 1344, 1376, 1377, 1378, 1379} <= set(e) and max(e) == 1380
  assert all({32 * t - 1, 32 * t, 32 * t + 1} <= set(e) for t in range(1, 44))
  e = hb.edge_positions(8300, 293, 128)                   # 3 tiles per split: split starts at multiples of 96
  assert {95, 96, 191, 192, 287, 288, 289, 290, 291, 292} <= set(e)


def test_live_pairs_cover_both_ends_and_a_chunk_boundary():
  assert hb.live_pairs(1) == () and hb.live_pairs(2) == ((0, 1), (1, 0)) and hb.live_pairs(4) == ((0, 3), (3, 0))
  for d in range(5, 129):
    (a, b), (k0, k1) = hb.live_pairs(d)
    assert (a, b) == (0, d - 1) and k1 == k0 + 1 < d and k0 % 2 == 1 and k0 // 4 + 1 == k1 // 4


# ------------------------------------------------------------------------------------------ windows
def _scores32(q, cand, reverse):
  """float32 scores by explicit float32 products summed feature by feature, forwards or backwards."""
  order = range(q.shape[1] - 1, -1, -1) if reverse else range(q.shape[1])
  s = np.zeros((q.shape[0], cand.shape[0]), np.float32)
  for k in order:
    if np.any(q[:, k]) and np.any(cand[:, k]):            # (a dead feature adds an exact 0)
      s += np.outer(q[:, k], cand[:, k]).astype(np.float32)
  assert s.dtype == np.float32
  return s


def _check_windows(case, nq, nc, d, full_coverage, products):
  """What every ``windows`` case is asked: the float64 reference equals the planted closed form, no positive is flagged,
  the canary beats every positive and the harmless row none, the positives are exact in float32 and every value lies
  under the bounds that make float32 exact.  ``products``: also the explicit float32 products over ALL queries, summed
  forwards and backwards, against float64 bit for bit."""
  assert np.array_equal(case["ref"], case["counts"]) and not case["ref_nonfinite"].any()
  centres, widths = case["centres"], case["widths"]
  if full_coverage:
    edges = hb.edge_positions(nq, nc, d)
    for w in hb.WIDTHS:
      assert set(edges) <= set(centres[widths == w].tolist()), w
    # the query that centres on an edge position with width 1 counts that candidate alone: dropping it shows
    solo = {int(c): b for b, (c, w) in enumerate(zip(centres, widths)) if w == 1}
    for e in edges:
      assert case["counts"][solo[e]] == 1
      moved = case["cand"].copy()
      moved[e] = case["harmless"]
      got, _ = hb.reference_counts(case["q"][solo[e]:solo[e] + 1], case["true_c"][solo[e]:solo[e] + 1], moved)
      assert got[0] == 0
  assert len(set(case["counts"].tolist())) >= min(nq, 4) - 1          # counts differ from query to query
  # bounds over all queries: the products 2 j centre and j^2 are integers below 2^24, every score
  # centre^2 - (j - centre)^2 and every positive an integer or half-integer below 2^23
  assert 2 * (nc - 1) * int(centres.max()) < 2 ** 24 and (nc - 1) ** 2 < 2 ** 23
  pos64 = (case["q"].astype(np.float64) * case["true_c"].astype(np.float64)).sum(axis=1)
  pos32 = (case["q"] * case["true_c"]).sum(axis=1, dtype=np.float32)
  assert np.array_equal(pos32.astype(np.float64), pos64) and np.abs(pos64).max() < 2 ** 23
  assert np.array_equal(pos64, centres.astype(np.float64) ** 2 - widths.astype(np.float64) ** 2 + (0.0 if case["tie"] else 0.5))
  if products:
    tied = 0
    for lo in range(0, nq, 2048):
      rows = slice(lo, min(lo + 2048, nq))
      s64 = case["q"][rows].astype(np.float64) @ case["cand"].astype(np.float64).T
      assert np.abs(s64).max() < 2 ** 23
      for reverse in (False, True):
        assert np.array_equal(_scores32(case["q"][rows], case["cand"], reverse).astype(np.float64), s64)
      tied += int((s64 == pos64[rows, None]).sum())
    # the candidates at distance width tie with the positive exactly (and only under ``tie``)
    inside = ((widths > 0) & (centres - widths >= 0)).sum() + ((widths > 0) & (centres + widths < nc)).sum() + (widths == 0).sum()
    assert tied == (inside if case["tie"] else 0)
  # the canary beats every positive, the harmless row none
  assert np.array_equal(hb.reference_counts(case["q"], case["true_c"], case["canary"][None])[0], np.ones(nq))
  assert np.array_equal(hb.reference_counts(case["q"], case["true_c"], case["harmless"][None])[0], np.zeros(nq))


@pytest.mark.parametrize("shape", SMALL_CASES + BIG_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_windows_cases_plant_what_they_say(shape):
  """All four variants (two placements, with and without ties) at every shape the GPU test uses.  Only the explicit
  float32 products are kept to one variant at the large shapes (the tied case on the chunk-straddling pair): the scores
  do not depend on the placement or on ``tie``, which moves the positives alone, and those are checked for every variant."""
  nq, nc, d = shape
  for family, pair in hb.families(d):
    if family == "grid":
      continue
    case = hb.build(family, nq, nc, d, pair)
    assert (case["k0"], case["k1"]) == hb.live_pairs(d)[pair] and case["tie"] == (family == "windows_tie")
    _check_windows(case, nq, nc, d, full_coverage=nq >= 4 * len(hb.edge_positions(nq, nc, d)),
                   products=shape not in BIG_CASES or (pair, family) == (1, "windows_tie"))


def test_every_corpus_size_has_a_case_that_covers_all_its_edges():
  covered = {nc for nq, nc, d in hb.layout_cases() if d >= 2 and nq >= 4 * len(hb.edge_positions(nq, nc, d))}
  assert {nc for _, nc, d in hb.layout_cases()} - covered == {1}      # (1 query; at 33 queries as many edges as fit, width 1 first)
  for nq, nc, d in ((1, 1, 4), (33, 40, 4)):
    c = hb.build("windows", nq, nc, d)
    edges = hb.edge_positions(nq, nc, d)
    assert set(edges) <= set(c["centres"][c["widths"] == 1].tolist())


def test_exactness_bound_of_the_windows_corpus():
  assert (hb.MAX_WINDOW_ROWS - 1) ** 2 + 0.5 < 2 ** 23                        # -j^2 and every positive
  assert 2 * (hb.MAX_WINDOW_ROWS - 1) ** 2 < 2 ** 24                          # the largest product 2 j centre
  assert max(nc for _, nc, _ in hb.layout_cases()) == hb.MAX_WINDOW_ROWS


# ------------------------------------------------------------------------------------------ grid
@pytest.mark.parametrize("shape", SMALL_CASES + BIG_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_grid_cases(shape):
  nq, nc, d = shape
  case = hb.build("grid", nq, nc, d)
  for x in (case["q"], case["true_c"], case["cand"]):
    assert np.array_equal(x * 4, np.round(x * 4)) and np.abs(x).max() <= 0.75
  assert np.array_equal(case["true_c"][case["copies"]], case["cand"][case["copied_rows"]]) and case["copies"].size >= 1
  assert not case["ref_nonfinite"].any()
  # explicit float32 products of the first 700 queries (a limit of this check; every value is a multiple of 1 / 4 of
  # magnitude <= 3 / 4 in all rows, asserted above, so every partial sum is a multiple of 1 / 16 below d 9 / 16 <= 72)
  s64 = case["q"][:700].astype(np.float64) @ case["cand"].astype(np.float64).T
  for reverse in (False, True):
    assert np.array_equal(_scores32(case["q"][:700], case["cand"], reverse).astype(np.float64), s64)
  assert np.array_equal(hb.reference_counts(case["q"], case["true_c"], case["canary"][None])[0], np.ones(nq))
  assert np.array_equal(hb.reference_counts(case["q"], case["true_c"], case["harmless"][None])[0], np.zeros(nq))
  # The two checks below need more than one feature, and enough queries for some count to move: they run at every grid
  # case with d >= 2 and at least 33 queries.  The cases left out are d = 1 and the one-query shape (1, 1).
  if d >= 2 and nq >= 33:
    # a coordinate paired with the wrong partner shows: swap two features of the candidates (neighbours, an even / odd
    # plane pair, the two ends)
    for a, b in {(0, 1), (0, d - 1), (d // 2, d // 2 - 1)}:
      swapped = case["cand"].copy()
      swapped[:, [a, b]] = swapped[:, [b, a]]
      assert not np.array_equal(hb.reference_counts(case["q"], case["true_c"], swapped)[0], case["ref"]), (a, b)
    # moving any single candidate away from an edge position (to a row that beats nobody) changes at least one count
    pos = (case["q"].astype(np.float64) * case["true_c"].astype(np.float64)).sum(axis=1)
    edges = hb.edge_positions(nq, nc, d)
    beats = case["q"].astype(np.float64) @ case["cand"][edges].astype(np.float64).T > pos[:, None]
    assert beats.any(axis=0).all()


# ------------------------------------------------------------------------------------------ ids, canaries
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("shape", [s for s in hb.ID_GEOMETRIES if s[0] <= 130], ids=lambda v: str(v).replace(" ", ""))
def test_with_ids_does_what_it_says(shape, id_dtype):
  nq, nc, d = shape
  for family, pair in hb.families(d)[-2:]:                  # a tied windows case (d >= 2) and the grid
    base = hb.build(family, nq, nc, d, pair)
    vocab = nc + 37
    case = hb.with_ids(base, vocab, id_dtype, hb.case_rng("ids", nq, nc, d))
    ids, table = case["ids"], case["table"]
    assert ids.dtype == id_dtype and table.shape == (vocab, d) and ids.shape == (nc,)
    wide = ids.astype(np.int64)
    valid = (wide >= 0) & (wide < vocab)
    kinds = [m[0] for m in case["mods"]]
    assert "negative" in kinds and (nc < 2 or "vocab" in kinds) and (nc < 4 or "dup" in kinds)
    assert (nc < 4 or id_dtype != np.int64 or "wide" in kinds) and np.array_equal(case["zero_rows"], np.flatnonzero(~valid))
    named = set(wide[valid].tolist())
    for r in range(vocab):
      if r not in named:
        assert np.array_equal(table[r], base["canary"])     # every row no id names is a canary
    touched = set()
    for what, at in case["mods"]:
      touched.add(at)
      if what == "negative":
        assert wide[at] == -1
      elif what == "vocab":
        assert wide[at] == vocab
      elif what == "wide":                                  # truncated to 32 bits it would name a canary
        assert wide[at] >= 2 ** 32 and np.array_equal(table[wide[at] & 0xFFFFFFFF], base["canary"])
      else:
        assert wide[at] == wide[at + 1] and np.array_equal(case["cand"][at], base["cand"][at + 1])
    keep = np.array([j for j in range(nc) if j not in touched], np.int64)
    assert np.array_equal(case["cand"][keep], base["cand"][keep]) and not case["cand"][case["zero_rows"]].any()
    # a zero row scores 0: it beats exactly the negative positives
    zero_beats = hb.reference_counts(base["q"], base["true_c"], np.zeros((1, d), np.float32))[0]
    assert np.array_equal(zero_beats, case["negative"].astype(np.int64))
    if family != "grid" and nq >= 33:
      assert case["negative"].any() and not case["negative"].all()
    # the reference of the scattered case, row by row: the base's counts with the touched rows exchanged
    want = hb.reference_counts(base["q"], base["true_c"], base["cand"][keep])[0] if keep.size else np.zeros(nq, np.int64)
    want = want + hb.reference_counts(base["q"], base["true_c"], case["cand"][sorted(touched)])[0]
    assert np.array_equal(hb.with_reference(case)["ref"], want)


def test_canary_tail_keeps_the_prefix_and_would_show():
  base = hb.build("windows", 130, 229, 7)
  case = hb.with_canary_tail(base, 40)
  assert case["alloc"].shape == (269, 7) and np.array_equal(case["alloc"][:229], base["cand"])
  assert np.array_equal(case["alloc"][229:], np.tile(base["canary"], (40, 1)))
  got = hb.reference_counts(base["q"], base["true_c"], case["alloc"][:230])[0]      # one row too many: every count moves
  assert np.array_equal(got, base["ref"] + 1)


# ------------------------------------------------------------------------------------------ in-batch, hits
def test_inbatch_windows_reference():
  q, c, counts = hb.inbatch_windows(300, 450, 12, 3, 4, hb.case_rng("inbatch", 300, 450, 12))
  ref, nonfinite = hb.reference_counts(q, c[:300], c)
  assert np.array_equal(ref, counts) and not nonfinite.any()
  assert {0, 1, 3, 65} <= set(counts.tolist())


def test_hits_inputs_and_reference():
  for nq in hb.HITS_NQ:
    counts, w = hb.hits_inputs(nq, True)
    low = counts & np.uint32(hb.COUNT_MASK)
    assert low.max() <= 20 and np.array_equal(w * 4, np.round(w * 4)) and (nq < 9 or (w == 0).any())
    if nq >= 1023:
      assert set(low.tolist()) == set(range(21)) and (counts >> 31).any() and not (counts >> 31).all()
    for nks, ks in hb.HITS_KS.items():
      assert len(ks) == nks and list(ks) != sorted(ks) or nks == 1
      hits, state = hb.hits_reference(counts, ks, w)
      assert np.array_equal(state.astype(np.float32).astype(np.float64), state)       # exact in float32 ...
      assert np.all(state * 4 == np.round(state * 4)) and state.max() * 4 < 2 ** 24      # ... in any order of summation
      assert not hits[:, (counts >> 31) == 1].any()
  assert 2 ** 31 - 1 in hb.HITS_KS[5] and 2 ** 31 - 1 in hb.HITS_KS[16]
  assert any(k in range(1, 21) for k in hb.HITS_KS[16])                                  # ks that equal some count
