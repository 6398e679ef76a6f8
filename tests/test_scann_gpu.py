"""factorized_top_k.ScaNN on the GPU: the reference's test grid and ScaNN tests (layers/factorized_top_k_test.py
:186-258), exactness against BruteForce when every leaf is searched and re-ordered, the kernels against the float64
restatement (tests/scann_restatement.py) within the bound of include/tfrs_hip.h, and the call surface."""

import numpy as np
import pytest

from oracle import topk as o_topk
from tests import scann_restatement as rs
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRID = load_golden("topk_grid.json")


def _ftk():
  from recommenders_amd.layers import factorized_top_k
  return factorized_top_k


def _np(x):
  return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _clustered(n, d, seed, centres=None):
  """A Gaussian mixture shaped like tools/bench_clustered.py's (unit-scale centres, 0.35 spread around them) but with
  UNIFORM cluster popularity (that tool draws Zipf(1) weights)."""
  rng = np.random.default_rng(seed)
  c = centres if centres is not None else max(1, n // 100)
  mu = rng.normal(size=(c, d)) / np.sqrt(d)
  cl = rng.integers(0, c, size=n)
  return (mu[cl] + 0.35 * rng.normal(size=(n, d)) / np.sqrt(d)).astype(np.float32)


class _Dataset:
  def __init__(self, candidates, ids, bs):
    self.c, self.i, self.bs = candidates, ids, bs

  def __iter__(self):
    for lo in range(0, self.c.shape[0], self.bs):
      if self.i is None:
        yield self.c[lo:lo + self.bs]
      else:
        yield (self.i[lo:lo + self.bs], self.c[lo:lo + self.bs])


@pytest.mark.parametrize("case", GRID["cases"],
                         ids=lambda c: "k{k}-b{batch_size}-q{num_queries}-n{num_candidates}-{indices_dtype}-x{use_exclusions}".format(**c))
def test_reference_grid(case):
  """test_scann_top_k (:245-258): one leaf, searched, every candidate re-ordered -- indices exact, scores bit-equal to
  the oracle's fma chain."""
  rng = np.random.RandomState(GRID["seed"])
  nc, nq = case["num_candidates"], case["num_queries"]
  candidates = rng.normal(size=(nc, GRID["dim"])).astype(np.float32)
  query = rng.normal(size=(nq, GRID["dim"])).astype(np.float32)
  exclude = rng.randint(0, nc, size=(nq, 5))
  ids = np.arange(nc).astype(str if case["indices_dtype"] == "str" else np.int32)
  with_ids = case["indices_dtype"] is not None
  layer = _ftk().ScaNN(k=case["k"], num_leaves=1, num_leaves_to_search=1, num_reordering_candidates=nc)
  for _ in range(2):
    layer.index_from_dataset(_Dataset(candidates, ids if with_ids else None, case["batch_size"]))
    if case["use_exclusions"]:
      top_scores, top_ids = layer.query_with_exclusions(query, ids[exclude])
    else:
      top_scores, top_ids = layer(query)
  expected_idx = np.asarray(case["expected_indices"])
  top_scores, top_ids = _np(top_scores), _np(top_ids)
  assert top_scores.shape == expected_idx.shape
  np.testing.assert_array_equal(top_ids.astype(ids.dtype), ids[expected_idx])
  np.testing.assert_array_equal(top_scores, np.take_along_axis(o_topk.scores(query, candidates), expected_idx, 1))


@pytest.mark.parametrize("dtype", ["str", "float32", "float64", "int32", "int64"])
def test_scann_reference_test(dtype, tmp_path):
  """test_scann (:186-214): 1000 x 4 rows, default parameters, identifiers of every dtype; repeated calls and a
  save / load round trip give identical results."""
  ftk = _ftk()
  rng = np.random.default_rng(0)
  candidates = rng.normal(size=(1000, 4)).astype(np.float32)
  query = rng.normal(size=(2, 4)).astype(np.float32)
  ids = np.arange(1000).astype(dtype)
  layer = ftk.ScaNN().index(candidates, ids)
  s0, i0 = layer(query)
  s0, i0 = _np(s0), _np(i0)
  assert s0.shape == (2, 10) and i0.shape == (2, 10)
  assert len(set(i0[0].tolist())) == 10
  for _ in range(100):
    s, i = layer(query)
    np.testing.assert_array_equal(_np(s), s0)
    np.testing.assert_array_equal(_np(i), i0)
  path = str(tmp_path / "scann.npz")
  layer.save(path)
  loaded = ftk.ScaNN.load(path)
  s, i = loaded(query)
  np.testing.assert_array_equal(_np(s), s0)
  np.testing.assert_array_equal(_np(i), i0)
  for key, val in layer.state_dict().items():
    other = loaded.state_dict()[key]
    if isinstance(val, np.ndarray):
      np.testing.assert_array_equal(val, other)
    else:
      assert val == other, key


@pytest.mark.parametrize("with_ids", [False, True])
def test_scann_dataset_forms(with_ids):
  """test_scann_dataset_arg_no_identifiers / _with_identifiers (:216-243)."""
  rng = np.random.default_rng(1)
  candidates = rng.normal(size=(100, 4)).astype(np.float32)
  ids = np.arange(100).astype(str) if with_ids else None
  layer = _ftk().ScaNN().index_from_dataset(_Dataset(candidates, ids, 10))
  s, i = layer(rng.normal(size=(3, 4)).astype(np.float32))
  assert tuple(s.shape) == (3, 10) and len(i) == 3


def test_scann_mismatched_identifiers_raise():
  rng = np.random.default_rng(2)
  candidates = rng.normal(size=(100, 4)).astype(np.float32)
  with pytest.raises(ValueError, match="same number of"):
    _ftk().ScaNN().index(candidates, np.arange(99))
  with pytest.raises(ValueError, match="same batch dimension"):
    _ftk().ScaNN().index_from_dataset([(np.arange(9), candidates[:10])])
  with pytest.raises(ValueError, match="2D"):
    _ftk().ScaNN().index(candidates[0])
  bad = candidates.copy()
  bad[3, 1] = np.nan
  with pytest.raises(ValueError, match="NaN"):
    _ftk().ScaNN().index(bad)


@pytest.mark.parametrize("d,dpb", [(64, 2), (3, 1), (20, 2), (100, 3), (128, 4), (64, 1), (64, 3), (20, 8)])
def test_every_leaf_reordered_equals_bruteforce(d, dpb):
  """All leaves searched, every probed row re-ordered: the result is BruteForce's, indices and scores."""
  ftk = _ftk()
  rng = np.random.default_rng(d * 10 + dpb)
  c = (rng.normal(size=(1000, d)) / np.sqrt(d)).astype(np.float32)
  q = (rng.normal(size=(50, d)) / np.sqrt(d)).astype(np.float32)
  layer = ftk.ScaNN(k=10, num_leaves=10, num_leaves_to_search=10, num_reordering_candidates=1000,
                    dimensions_per_block=dpb).index(c)
  s, i = layer(q)
  bs, bi = ftk.BruteForce(k=10).index(c)(q)
  np.testing.assert_array_equal(_np(i), _np(bi))
  np.testing.assert_array_equal(_np(s), _np(bs))


_BIG = {}


def _big_layer(reorder):
  if reorder not in _BIG:
    c = _clustered(200_000, 64, 7, centres=2000)
    layer = _ftk().ScaNN(k=10, num_leaves=2000, num_leaves_to_search=40,
                         num_reordering_candidates=500 if reorder else None).index(c)
    _BIG[reorder] = (c, layer, layer.state_dict())
  return _BIG[reorder]


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("nq", [1, 7, 300])
def test_kernels_against_restatement(reorder, nq):
  """Clustered 200 k x 64, 2000 leaves, 40 searched: the probe sets are the restatement's; without re-ordering every
  returned s~ is within the header's bound of the float64 score of the decoded vector and the rows are the top k up to
  that band; with re-ordering (R = 500) the scores are the oracle's fma chain and the rows the exact top k of the
  top-R candidate set, up to the band at the R cut."""
  c, layer, st = _big_layer(reorder)
  k = 10
  q = _clustered(nq, 64, 1000 + nq, centres=50)
  s, rows = layer(q)
  s, rows = _np(s), _np(rows)
  l_eff, p_max, probe_idx, probe_s = rs.probes(st, q, k, 40)
  assert layer.probe_plan(k) == (l_eff, p_max)
  got_s, got_leaves = layer.probe_leaves(q, k)           # the probe sets ARE the restatement's
  np.testing.assert_array_equal(_np(got_leaves), probe_idx)
  np.testing.assert_array_equal(_np(got_s), probe_s)
  exact = o_topk.scores(q, c) if reorder else None
  for b in range(nq):
    orig, s64, eps = rs.candidates(st, q[b], probe_idx[b])
    where = {int(r): j for j, r in enumerate(orig)}
    assert len(set(rows[b].tolist())) == k
    assert all(int(r) in where for r in rows[b]), "a returned row is outside the probed leaves"
    j = np.asarray([where[int(r)] for r in rows[b]])
    if not reorder:
      assert np.all(np.abs(s[b].astype(np.float64) - s64[j]) <= eps[j]), b
      sure = np.flatnonzero(rs.surely_in(s64, eps, k))
      assert set(orig[sure].tolist()) <= set(rows[b].tolist()), b
      assert np.all(rs.possibly_in(s64, eps, k)[j]), b
    else:
      np.testing.assert_array_equal(s[b], exact[b, rows[b]])
      key = sorted(zip((-exact[b, rows[b]]).tolist(), rows[b].tolist()))
      assert [r for _, r in key] == rows[b].tolist()
      assert np.all(rs.possibly_in(s64, eps, 500)[j]), b
      sure = rs.surely_in(s64, eps, 500)
      kth = (-float(s[b, -1]), int(rows[b, -1]))
      better = [int(orig[t]) for t in np.flatnonzero(sure) if (-float(exact[b, orig[t]]), int(orig[t])) < kth]
      assert set(better) <= set(rows[b].tolist()), b


def test_probe_widening():
  """Leaves so uneven that num_leaves_to_search leaves can hold fewer than k rows: every result is a real, distinct
  row and the shape is [B, k].  The corpus has exactly 9 distinct rows (8 single ones, one repeated 2000 times), so
  9 leaves are those rows whatever the initial order: leaf sizes 1 x 8 and 2000."""
  ftk = _ftk()
  rng = np.random.default_rng(3)
  d = 8
  far = np.eye(d, dtype=np.float32) * 100.0
  c = np.concatenate([far, np.full((2000, d), 0.01, dtype=np.float32)])
  c = c[rng.permutation(len(c))]
  layer = ftk.ScaNN(k=50, num_leaves=9, num_leaves_to_search=2, training_iterations=4).index(c)
  assert sorted(np.diff(layer.state_dict()["leaf_offsets"]).tolist()) == [1] * 8 + [2000]
  l_eff, p_max = layer.probe_plan()
  assert (l_eff, p_max) == (9, 2008)
  s, i = layer(rng.normal(size=(20, d)).astype(np.float32))
  s, i = _np(s), _np(i)
  assert i.shape == (20, 50)
  assert np.all(np.isfinite(s))
  assert np.all((i >= 0) & (i < c.shape[0]))
  assert all(len(set(r.tolist())) == 50 for r in i)


def test_index_is_deterministic():
  c = _clustered(20_000, 32, 11)
  a = _ftk().ScaNN(num_leaves=50, num_reordering_candidates=100, seed=5).index(c).state_dict()
  b = _ftk().ScaNN(num_leaves=50, num_reordering_candidates=100, seed=5).index(c).state_dict()
  for key, val in a.items():
    if isinstance(val, np.ndarray):
      np.testing.assert_array_equal(val, b[key])
    else:
      assert val == b[key], key


@pytest.mark.parametrize("reorder", [None, 200])
def test_scale_invariance(reorder):
  """Candidates x 2^30 and queries x 2^-20: the same rows, re-ordered scores exactly 2^10 times (an fp16 overflow or
  flush in the scan would change the rows)."""
  ftk = _ftk()
  c = _clustered(20_000, 64, 13)
  q = _clustered(64, 64, 14)
  kw = dict(k=20, num_leaves=100, num_leaves_to_search=10, num_reordering_candidates=reorder)
  s1, i1 = ftk.ScaNN(**kw).index(c)(q)
  s2, i2 = ftk.ScaNN(**kw).index(c * np.float32(2.0 ** 30))(q * np.float32(2.0 ** -20))
  np.testing.assert_array_equal(_np(i1), _np(i2))
  if reorder is not None:
    np.testing.assert_array_equal(_np(s2), _np(s1) * np.float32(2.0 ** 10))


def test_call_surface():
  ftk = _ftk()
  c = _clustered(5000, 16, 17)
  q = _clustered(8, 16, 18)
  layer = ftk.ScaNN(k=10, num_leaves=20, num_leaves_to_search=5, num_reordering_candidates=100)
  with pytest.raises(ValueError, match="index"):
    layer(q)
  layer.index(c)
  s, i = layer(q[0])
  assert tuple(s.shape) == (10,) and tuple(i.shape) == (10,)
  sb, ib = layer(q)
  np.testing.assert_array_equal(_np(i), _np(ib)[0])
  s5, _ = layer(q, k=5)
  assert tuple(s5.shape) == (8, 5)
  with pytest.raises(ValueError):
    layer(q, k=5001)
  with pytest.raises(ValueError, match="1024"):
    ftk.ScaNN(k=10, num_leaves=1).index(_clustered(3000, 16, 19))(q, k=1025)
  with pytest.raises(ValueError, match="rank"):
    layer(q[None])
  model = lambda x: x * 2.0
  lm = ftk.ScaNN(query_model=model, k=10, num_leaves=20, num_leaves_to_search=5, num_reordering_candidates=100)
  lm.load_state_dict(layer.state_dict())
  s2, i2 = lm(torch.as_tensor(q).cuda())
  s3, i3 = layer(q * 2.0)
  np.testing.assert_array_equal(_np(i2), _np(i3))
  np.testing.assert_array_equal(_np(s2), _np(s3))
  # exclusions: the top k + E of the plain search, excluded identifiers removed
  excl = _np(ib)[:, :3]
  se, ie = layer.query_with_exclusions(q, excl, k=5)
  full_s, full_i = layer(q, k=8)
  for b in range(8):
    keep = [r for r in _np(full_i)[b] if r not in set(excl[b].tolist())][:5]
    assert _np(ie)[b].tolist() == keep


def test_exclusions_against_restatement():
  """query_with_exclusions (:242-288) against the restatement: with R >= P_max every probed row is re-ordered, so
  the answer is the oracle's exclusion step over the exact scores of the restatement's probed rows."""
  ftk = _ftk()
  c = _clustered(2000, 16, 41)
  q = _clustered(8, 16, 42)
  ids = (np.arange(2000) * 7 + 3).astype(np.int64)
  layer = ftk.ScaNN(k=10, num_leaves=20, num_leaves_to_search=5, num_reordering_candidates=1024).index(c, ids)
  st = layer.state_dict()
  k, e = 5, 3
  l_eff, p_max, probe_idx, _ = rs.probes(st, q, k + e, 5)
  assert p_max <= 1024
  exact = o_topk.scores(q, c)
  rng = np.random.default_rng(43)
  excl = np.stack([rng.choice(ids, size=e, replace=False) for _ in range(8)])
  want_s, want_i = [], []
  for b in range(8):
    rows, _, _ = rs.candidates(st, q[b], probe_idx[b])
    order = sorted(rows.tolist(), key=lambda r: (-exact[b, r], r))[:k + e]
    ws, wi = o_topk.exclude(exact[b, order][None], ids[order][None], excl[b][None], k)
    want_s.append(ws[0])
    want_i.append(wi[0])
  s, i = layer.query_with_exclusions(q, excl, k=k)
  np.testing.assert_array_equal(_np(i), np.stack(want_i))
  np.testing.assert_array_equal(_np(s), np.stack(want_s))


def test_metric_matches_bruteforce_when_exact():
  ftk = _ftk()
  from recommenders_amd import metrics
  rng = np.random.default_rng(21)
  c = (rng.normal(size=(1000, 16)) / 4).astype(np.float32)
  q = (rng.normal(size=(64, 16)) / 4).astype(np.float32)
  true_ids = rng.integers(0, 1000, size=64)
  scann = ftk.ScaNN(k=100, num_leaves=10, num_leaves_to_search=10, num_reordering_candidates=1000).index(c)
  bf = ftk.BruteForce(k=100).index(c)
  got, want = [], []
  for layer, out in ((scann, got), (bf, want)):
    m = metrics.FactorizedTopK(candidates=layer, ks=(1, 5, 10, 50, 100))
    m.update_state(torch.as_tensor(q).cuda(), torch.as_tensor(c[true_ids]).cuda(),
                   true_candidate_ids=torch.as_tensor(true_ids).cuda())
    out.extend(float(v) for v in m.result())
  assert got == want
  with pytest.raises(ValueError, match="true_candidate_ids"):
    metrics.FactorizedTopK(candidates=scann).update_state(torch.as_tensor(q).cuda(),
                                                          torch.as_tensor(c[true_ids]).cuda())


@pytest.mark.parametrize("reorder", [None, 300])
def test_chunking(reorder, monkeypatch):
  ftk = _ftk()
  c = _clustered(50_000, 32, 23)
  q = _clustered(300, 32, 24)
  layer = ftk.ScaNN(k=10, num_leaves=200, num_leaves_to_search=20, num_reordering_candidates=reorder).index(c)
  s1, i1 = layer(q)
  _, p_max = layer.probe_plan()
  from recommenders_amd import _lib
  from recommenders_amd.layers.factorized_top_k import scann as scann_module   # (the module that reads the budget)
  lib, search, sizes = _lib.load(), _lib.load().tfrs_scann_search, []

  def counted_search(queries, nq, *rest):
    sizes.append(nq)
    return search(queries, nq, *rest)

  monkeypatch.setattr(lib, "tfrs_scann_search", counted_search)
  layer(q)
  assert sizes == [300]                                                    # the default budget: one chunk
  del sizes[:]
  monkeypatch.setattr(scann_module, "_SCANN_SCORE_BUDGET_BYTES", 4 * p_max * 100)   # 100 queries per chunk: 3 chunks
  s2, i2 = layer(q)
  assert sizes == [100, 100, 100]
  np.testing.assert_array_equal(_np(i1), _np(i2))
  np.testing.assert_array_equal(_np(s1), _np(s2))


@pytest.mark.parametrize("nq", [1, 64])
def test_graph_replay(nq):
  ftk = _ftk()
  c = _clustered(50_000, 64, 25)
  q = _clustered(nq, 64, 26)
  layer = ftk.ScaNN(k=10, num_leaves=200, num_leaves_to_search=20, num_reordering_candidates=200).index(c)
  s0, i0 = layer(q)
  s0, i0 = _np(s0).copy(), _np(i0).copy()
  graphed = layer.make_graphed_call(q)
  for _ in range(3):
    s, i = graphed(q)
    np.testing.assert_array_equal(_np(s), s0)
    np.testing.assert_array_equal(_np(i), i0)


def test_recall_floor():
  """Clustered 1 M x 64, 1000 leaves, 100 searched, 1000 re-ordered, 1000 queries: recall@10 against BruteForce.
  A guard against a broken trainer: an MI355X run observed 0.669 (0.645 while the k-means started from the lowest
  sampled rows; this mixture has 10 000 centres of 100 rows, finer than the 1000 leaves); the floor keeps a margin
  below it."""
  ftk = _ftk()
  c = _clustered(1_000_000, 64, 31, centres=10_000)
  q = _clustered(1000, 64, 32, centres=10_000)
  layer = ftk.ScaNN(k=10, num_leaves=1000, num_leaves_to_search=100, num_reordering_candidates=1000).index(c)
  _, i = layer(q)
  _, bi = ftk.BruteForce(k=10).index(c)(q)
  i, bi = _np(i), _np(bi)
  recall = np.mean([len(set(i[b].tolist()) & set(bi[b].tolist())) / 10.0 for b in range(len(q))])
  print("recall@10", recall)
  assert recall >= RECALL_FLOOR, recall


RECALL_FLOOR = 0.55
