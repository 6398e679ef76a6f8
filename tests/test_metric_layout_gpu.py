"""The rank-count metric kernels (csrc/metric_fused.hip: ``rank_count_kernel<DP>``, ``hits_update_kernel``) and the two
small per-query kernels of csrc/topk_api.hip (``rank_of_positive_kernel``, ``id_match_kernel``), checked PER QUERY on
the hand-built corpora of tests/metric_handbuilt.py: the ``counts`` buffer itself (read through the C entry points,
before ``tfrs_topk_hits_update`` re-arms it) equals the float64 reference for every query by exact integer equality,
and bit 31 equals the reference's "positive not finite".  tests/test_metric_handbuilt_host.py proves on the host that
every case has the geometry it claims (tiles per split, splits, ragged last split and tile), that the inputs are exact
in float32 in any summation order, and that the reference equals what the builders planted.

The ``windows`` family needs two live coordinates: at d = 1 only ``grid`` runs."""

import ctypes

import numpy as np
import pytest

from tests import metric_handbuilt as hb

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEAN_RTOL = 2e-6        # tests/test_ops_gpu.py: the bound of the rank-count metric means


def _t(a, **kw):
  return torch.as_tensor(np.ascontiguousarray(a), **kw).cuda()


def _assert_counts(tag, raw, ref, nonfinite=None):
  low, flag = (raw & np.uint32(hb.COUNT_MASK)).astype(np.int64), (raw >> np.uint32(31)).astype(bool)
  bad = np.flatnonzero(low != ref)
  assert bad.size == 0, f"{tag}: {bad.size} queries differ, first {bad[:8]}: got {low[bad[:8]]}, want {ref[bad[:8]]}"
  want_flag = np.zeros(ref.shape, bool) if nonfinite is None else nonfinite
  assert np.array_equal(flag, want_flag), f"{tag}: bit 31 differs at {np.flatnonzero(flag != want_flag)[:8]}"


def _run_families(nq, nc, d):
  for family, pair in hb.families(d):
    case = hb.build(family, nq, nc, d, pair)
    raw, _ = hb.device_counts(case["q"], case["true_c"], case["cand"])
    _assert_counts(f"{family}[{pair}] {(nq, nc, d)}", raw, case["ref"], case["ref_nonfinite"])


# ------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("shape", [(nq, nc, d) for (nq, nc), dims, _ in hb.GEOMETRIES for d in dims],
                         ids=lambda v: str(v).replace(" ", ""))
def test_counts_at_every_geometry(shape):
  _run_families(*shape)


@pytest.mark.parametrize("shape", list(hb.DEPTH_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_counts_at_every_number_of_tiles_per_split(shape):
  assert hb.plan(*shape)[1] == hb.DEPTH_SHAPES[shape]
  _run_families(*shape)


@pytest.mark.parametrize("d", hb.DIM_SWEEP)
def test_counts_over_the_dim_sweep(d):
  _run_families(*hb.DIM_SWEEP_SHAPE, d)


@pytest.mark.parametrize("nq", hb.QUERY_EDGE_NQ)
def test_counts_at_query_side_edges(nq):
  _run_families(nq, hb.QUERY_EDGE_NC, hb.QUERY_EDGE_D)


@pytest.mark.parametrize("shape", hb.ID_GEOMETRIES, ids=lambda v: str(v).replace(" ", ""))
def test_counts_through_ids_and_beside_canaries(shape):
  """Every table row no id names, and every row past nc of the allocation, would beat every positive: one read of a
  wrong row moves a count.  Out-of-range ids (-1, vocab, 2^32 + a canary's row) score as zero rows, which beat the
  negative positives."""
  nq, nc, d = shape
  for family, pair in hb.families(d)[-2:]:
    base = hb.build(family, nq, nc, d, pair)
    for id_dtype in (np.int32, np.int64):
      case = hb.with_reference(hb.with_ids(base, nc + 37, id_dtype, hb.case_rng("ids", nq, nc, d)))
      raw, _ = hb.device_counts(case["q"], case["true_c"], case["table"], ids=case["ids"], vocab=case["vocab"])
      _assert_counts(f"ids {family} {np.dtype(id_dtype).name} {shape}", raw, case["ref"])
      if family != "grid" and nq >= 130:
        assert np.any(case["ref"] != base["ref"])            # (the zero rows do count somewhere)
    tail = hb.with_canary_tail(base, 40)
    raw, _ = hb.device_counts(tail["q"], tail["true_c"], tail["alloc"], nc=nc)
    _assert_counts(f"tail {family} {shape}", raw, base["ref"])


# ------------------------------------------------------------------------------------------ blocks
@pytest.mark.parametrize("family,d", [("windows", 12), ("windows_tie", 7), ("grid", 7), ("grid", 16)])
def test_block_sweep_equals_one_launch_and_a_second_sweep_doubles(family, d):
  nq, nc = 300, sum(hb.BLOCK_ROWS)
  case = hb.build(family, nq, nc, d, 1 if family != "grid" else 0)
  single, _ = hb.device_counts(case["q"], case["true_c"], case["cand"])
  _assert_counts("single", single, case["ref"])
  buf = None
  for sweep in (1, 2):
    lo = 0
    for i, rows in enumerate(hb.BLOCK_ROWS):
      raw, buf = hb.device_counts(case["q"], case["true_c"], case["cand"][lo:lo + rows].copy(),
                                  first_block=1 if i == 0 else 0, counts=buf)
      lo += rows
    assert lo == nc
    _assert_counts(f"sweep {sweep}", raw, sweep * case["ref"])          # not re-armed: the second sweep adds


# ------------------------------------------------------------------------------------------ non-finite positives
@pytest.mark.parametrize("shape", hb.NONFINITE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_nonfinite_positives_are_flagged_exactly_once(shape):
  nq, nc, d = shape
  base = hb.build("windows", nq, nc, d, 0)
  true_c = base["true_c"].copy()
  k1 = base["k1"]
  rows = [0, 1, 2, 31, 127, nq // 2, nq - 3, nq - 2, nq - 1]            # first and last query tile, and between
  values = [np.inf, -np.inf, np.nan]
  for i, b in enumerate(rows):
    true_c[b, k1] = values[i % 3]                                       # q[b, k1] = 1: the scores stay finite
  ref, nonfinite = hb.reference_counts(base["q"], true_c, base["cand"])
  assert np.array_equal(np.flatnonzero(nonfinite), sorted(rows)) and ref[1] == nc and ref[0] == 0 and ref[2] == 0
  raw, _ = hb.device_counts(base["q"], true_c, base["cand"], first_block=1)
  _assert_counts("first block", raw, ref, nonfinite)
  raw, _ = hb.device_counts(base["q"], true_c, base["cand"], first_block=0)
  _assert_counts("later block", raw, ref, None)                         # bit 31 nowhere
  # blocks: flagged by the first block only, once
  buf, lo = None, 0
  for i, rows_b in enumerate((33, 64, nc - 97)):
    raw, buf = hb.device_counts(base["q"], true_c, base["cand"][lo:lo + rows_b].copy(), first_block=1 if i == 0 else 0,
                                counts=buf)
    lo += rows_b
  _assert_counts("blocks", raw, ref, nonfinite)


# ------------------------------------------------------------------------------------------ tfrs_topk_hits_update
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("nq", hb.HITS_NQ)
def test_hits_update_per_example(nq, weighted):
  counts, w = hb.hits_inputs(nq, weighted)
  for nks, ks in hb.HITS_KS.items():
    want_hits, want_state = hb.hits_reference(counts, ks, w)
    hits, state, results, after = hb.device_hits_update(counts, ks, w)
    assert hits.shape == (nks, nq) and np.array_equal(hits.astype(np.float64), want_hits), (nq, nks)
    assert not after.any()                                              # re-armed
    assert np.array_equal(state.astype(np.float64), want_state), (nq, nks)
    want_mean = np.where(want_state[nks:] > 0, want_state[:nks] / np.maximum(want_state[nks:], 0.25), 0.0)
    np.testing.assert_allclose(results, want_mean, rtol=MEAN_RTOL, atol=0)
    # the state accumulates over a second call (and the per-example output is optional)
    none, state2, results2, after = hb.device_hits_update(counts, ks, w, state=state, want_hits=False)
    assert none is None and not after.any() and np.array_equal(state2.astype(np.float64), 2 * want_state)
    np.testing.assert_allclose(results2, want_mean, rtol=MEAN_RTOL, atol=0)
    zeros = np.zeros(nq, np.float32)
    hits, state, results, _ = hb.device_hits_update(counts, ks, zeros)
    assert np.array_equal(hits.astype(np.float64), want_hits) and not state.any() and np.array_equal(results, np.zeros(nks))


# ------------------------------------------------------------------------------------------ the list kernels
LIST_KMAX = (1, 63, 64, 65, 130)
LIST_NQ = (1, 3, 4, 5)


def _list_ks(kmax):
  ks = [kmax, 1, kmax + 1, 2 ** 31 - 1, 2, 64, 63, 65, max(kmax - 1, 1), 3, 33, 32, 129, 130, 131, 7]
  assert len(ks) == 16
  return ks


@pytest.mark.parametrize("kmax", LIST_KMAX)
@pytest.mark.parametrize("nq", LIST_NQ)
def test_rank_of_positive_per_example(nq, kmax):
  """Sorted lists with pairs of equal entries; positives tied with entries at the first, the last and a middle column,
  above and below the whole list, and not finite."""
  from recommenders_amd import _lib
  lib = _lib.load()
  ks = _list_ks(kmax)
  cols = np.arange(kmax)
  topk = np.stack([((kmax - cols + 1) // 2 + b).astype(np.float32) for b in range(nq)])     # descending, ties in pairs
  assert np.all(np.diff(topk, axis=1) <= 0)
  q = np.tile(np.array([1.0, 0.5, 2.0], np.float32), (nq, 1))
  c = np.zeros((nq, 3), np.float32)
  for variant in range(3):
    choose = [topk[:, 0], topk[:, -1], topk[:, kmax // 2], topk[:, 0] + 1, topk[:, -1] - 1]
    c[:, 0] = [choose[(b + variant) % 5][b] for b in range(nq)]
    if variant == 2:
      c[:, 0] = [[np.inf, -np.inf, np.nan][b % 3] for b in range(nq)]
    with np.errstate(invalid="ignore"):
      pos = (q.astype(np.float64) * c.astype(np.float64)).sum(axis=1)
      greater = (topk.astype(np.float64) > pos[:, None]).sum(axis=1)
    want = np.stack([(np.isfinite(pos) & (greater < k)).astype(np.float32) for k in ks])
    out = torch.full((16, nq), -1.0, dtype=torch.float32, device="cuda")
    tq, tc, tk = _t(q), _t(c), _t(topk)
    _lib.check(lib.tfrs_rank_of_positive(_lib.ptr(tq), _lib.ptr(tc), nq, 3, _lib.ptr(tk), kmax,
                                         (ctypes.c_int32 * 16)(*ks), 16, _lib.ptr(out), _lib.current_stream()))
    assert np.array_equal(out.cpu().numpy(), want), (nq, kmax, variant)
    if variant == 2:
      assert not want.any()


@pytest.mark.parametrize("kmax", LIST_KMAX)
@pytest.mark.parametrize("nq", LIST_NQ)
def test_id_match_per_example(nq, kmax):
  """A match at column k - 1 (a hit at k), at column k (no hit at k), no match, and an id that appears twice."""
  from recommenders_amd import _lib
  lib = _lib.load()
  ks = _list_ks(kmax)
  for k_star in sorted({k for k in ks if k <= kmax}):
    ids = (1000 + 3 * np.arange(kmax)[None, :] + 7919 * np.arange(nq)[:, None]).astype(np.int32)
    true = np.zeros(nq, np.int32)
    for b in range(nq):
      scenario = (b + k_star) % 4
      if scenario == 0:
        true[b] = ids[b, k_star - 1]
      elif scenario == 1 and k_star < kmax:
        true[b] = ids[b, k_star]
      elif scenario == 3 and k_star < kmax:
        ids[b, kmax - 1] = ids[b, k_star]                   # duplicated: the earlier column decides
        true[b] = ids[b, k_star]
      else:
        true[b] = -5
    first = np.array([next((j for j in range(kmax) if ids[b, j] == true[b]), kmax) for b in range(nq)])
    want = np.stack([(first < k).astype(np.float32) for k in ks])
    out = torch.full((16, nq), -1.0, dtype=torch.float32, device="cuda")
    ti, tt = _t(ids), _t(true)
    _lib.check(lib.tfrs_id_match_topk(_lib.ptr(ti), _lib.ptr(tt), nq, kmax, (ctypes.c_int32 * 16)(*ks), 16,
                                      _lib.ptr(out), _lib.current_stream()))
    assert np.array_equal(out.cpu().numpy(), want), (nq, kmax, k_star)


# ------------------------------------------------------------------------------------------ Python level
PY_KS = (1, 2, 3, 4, 65, 66)          # straddle the planted window sizes 0, 1, 3, 65: one miscount flips a hit


def _weights(nq):
  return ((np.arange(nq) % 8 + 1) / 4.0).astype(np.float32)


def _want_means(ref, nonfinite, w, ks=PY_KS):
  w64 = w.astype(np.float64)
  return [float(((~nonfinite & (ref < k)) * w64).sum() / w64.sum()) for k in ks]


def _py_case():
  nq, nc, d = 300, 1381, 20
  base = hb.build("windows", nq, nc, d, 1)
  true_c = base["true_c"].copy()
  true_c[5, base["k1"]], true_c[nq - 1, base["k1"]] = np.nan, np.inf    # count 0: only the flag keeps them from hitting
  case = dict(base, true_c=true_c)
  ref, nonfinite = hb.reference_counts(case["q"], true_c, case["cand"])
  assert nonfinite.sum() == 2 and {0, 1, 3, 65} <= set(ref.tolist())
  return case, ref, nonfinite


def test_factorized_top_k_over_an_embedding_dataset_and_over_blocks():
  import recommenders_amd as tfrs
  from recommenders_amd.layers import embedding as emb
  case, _, _ = _py_case()
  nq, (nc, d) = case["q"].shape[0], case["cand"].shape
  w = _weights(nq)
  for id_dtype in (np.int32, np.int64):
    scattered = hb.with_ids(case, nc + 37, id_dtype, hb.case_rng("py", nq, nc, d))
    ref, nonfinite = hb.reference_counts(scattered["q"], scattered["true_c"], scattered["cand"])
    want = _want_means(ref, nonfinite, w)
    layer = emb.Embedding(scattered["vocab"], d).cuda()
    with torch.no_grad():
      layer.embeddings.copy_(_t(scattered["table"]))
    ds = tfrs.data.Dataset.from_tensor_slices(_t(scattered["ids"])).batch(128).map(layer)
    assert ds.as_embedding_rows() is not None
    blocks = [_t(scattered["cand"][lo:lo + 128]) for lo in range(0, nc, 128)]
    for name, src in (("dataset", ds), ("blocks", blocks)):
      metric = tfrs.metrics.FactorizedTopK(candidates=src, ks=PY_KS)
      metric.update_state(_t(case["q"]), _t(case["true_c"]), sample_weight=_t(w))
      np.testing.assert_allclose([float(v) for v in metric.result()], want, rtol=MEAN_RTOL, err_msg=name)
  assert want[0] < want[1] < want[3] < want[5]                          # every k separates some queries


def test_factorized_top_k_with_an_empty_first_block():
  """A candidate list whose first block has 0 rows: the launch that flags the non-finite positives is the first one
  that has rows.  The results equal those without the empty block."""
  import recommenders_amd as tfrs
  case, ref, nonfinite = _py_case()
  nq, (nc, d) = case["q"].shape[0], case["cand"].shape
  w = _weights(nq)
  want = _want_means(ref, nonfinite, w)
  blocks = [_t(case["cand"][lo:lo + 450]) for lo in range(0, nc, 450)]
  empty = torch.zeros((0, d), dtype=torch.float32, device="cuda")
  got = {}
  for name, src in (("plain", blocks), ("empty_first", [empty] + blocks), ("empty_middle", blocks[:1] + [empty] + blocks[1:])):
    metric = tfrs.metrics.FactorizedTopK(candidates=src, ks=PY_KS)
    metric.update_state(_t(case["q"]), _t(case["true_c"]), sample_weight=_t(w))
    got[name] = [float(v) for v in metric.result()]
    np.testing.assert_allclose(got[name], want, rtol=MEAN_RTOL, err_msg=name)
  assert got["empty_first"] == got["plain"] == got["empty_middle"]
  # what losing the flag would give: the two non-finite positives hit at every k
  lost = _want_means(ref, np.zeros_like(nonfinite), w)
  assert all(abs(a - b) > 1e-3 * b for a, b in zip(lost, want))


@pytest.mark.parametrize("k", PY_KS)
def test_batch_top_k_accuracy_from_embeddings(k):
  from recommenders_amd.tasks.retrieval import TopKCategoricalAccuracy
  nq, nc, d = 300, 450, 12
  q, c, counts = hb.inbatch_windows(nq, nc, d, 3, 4, hb.case_rng("inbatch", nq, nc, d))
  w = _weights(nq)
  want = _want_means(counts, np.zeros(nq, bool), w, ks=(k,))[0]
  metric = TopKCategoricalAccuracy(k=k)
  metric.update_from_embeddings(_t(q), _t(c), sample_weight=_t(w))
  assert float(metric.result()) == pytest.approx(want, rel=MEAN_RTOL)
  metric.update_from_embeddings(_t(q), _t(c), sample_weight=_t(w))     # running mean over two updates
  assert float(metric.result()) == pytest.approx(want, rel=MEAN_RTOL)
