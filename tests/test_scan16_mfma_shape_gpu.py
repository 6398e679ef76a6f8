"""The MFMA shape of the fp16 scan kernels (TFRS_SCAN16_MFMA = 32x32 | 16x16, csrc/topk_scan16.hip) changes which lane
holds which (query, candidate) score -- and with it the raw-score hook, the survivor queue, its drain and the bins of
the threshold pass.  Both arms are held to float64 score by score and to the all-f32 search batch by batch; nothing here
times anything or tries to break anything: results are compared."""
import numpy as np
import pytest
import torch

from oracle import topk as o_topk

pytestmark = pytest.mark.gpu
ARMS = ["32x32", "16x16"]


@pytest.fixture(params=ARMS)
def mfma(request):
  from recommenders_amd import _lib
  _lib.set_option("TFRS_SCAN16_MFMA", request.param)
  yield request.param
  _lib.set_option("TFRS_SCAN16_MFMA", None)


def test_the_switch_rejects_other_values():
  from recommenders_amd import _lib
  from recommenders_amd.layers import factorized_top_k as ftk
  c = torch.randn((70_000, 64), device="cuda") / 8
  layer = ftk.BruteForce(k=10).index(c)
  _lib.set_option("TFRS_SCAN16_MFMA", "16x16x32")
  try:
    with pytest.raises(ValueError, match="TFRS_SCAN16_MFMA"):
      layer(c[:4])
  finally:
    _lib.set_option("TFRS_SCAN16_MFMA", None)


@pytest.mark.parametrize("data", ["row_scales", "gauss"])
@pytest.mark.parametrize("d", [32, 48, 64, 100, 128])
def test_raw_prefilter_scores_sit_where_they_belong(d, data, mfma):
  """tfrs_debug_fp16_scores (the MATERIALIZE mode of scan16_kernel) against float64, element for element in the
  (query, row) position: |s16 - s| <= ||q|| N_stage * 0.00104 as tests/test_topk_gpu.py::test_f16_prefilter_error_bound
  asserts (kappa of common.h before its 5 % slack: the bound holds for any f32 accumulation order of the D
  products, so for both shapes).  A layout error is a permutation of scores between rows or queries, and with row
  norms that differ by orders of magnitude it misses this bound by orders of magnitude.  1317 rows (the last stage
  holds 37) and 203 queries (the last group of 32 holds 11)."""
  from recommenders_amd import _lib
  from recommenders_amd.layers import factorized_top_k as ftk
  rng = np.random.default_rng(700 + d)
  n, nq = 1317, 203
  if data == "row_scales":   # the data of test_f16_prefilter_error_bound
    scale = np.exp(rng.normal(size=(n, 1)) * 3.0)
    c = (rng.normal(size=(n, d)) * scale).astype(np.float32)
    c[:, ::3] *= np.float32(1e-5)
    q = (rng.normal(size=(nq, d)) * np.exp(rng.normal(size=(nq, 1)))).astype(np.float32)
    q[:, 1::4] *= np.float32(3e-6)
  else:
    c = (rng.normal(size=(n, d)) / np.sqrt(d)).astype(np.float32)
    q = (rng.normal(size=(nq, d)) / np.sqrt(d)).astype(np.float32)
  layer = ftk.BruteForce(k=10).index(c)
  ld = (n + 127) // 128 * 128
  out = torch.full((nq, ld), float("nan"), dtype=torch.float32, device="cuda")
  scratch = torch.empty((2 * nq,), dtype=torch.float32, device="cuda")
  tq = torch.as_tensor(q).cuda()
  lib = _lib.load()
  _lib.check(lib.tfrs_debug_fp16_scores(layer._index.handle, _lib.ptr(tq), nq, 0, n, _lib.ptr(out),
                                        _lib.ptr(scratch), _lib.current_stream()))
  got = out.cpu().numpy().astype(np.float64)
  assert np.isfinite(got).all()                              # every (query, row) slot was written
  exact = q.astype(np.float64) @ c.astype(np.float64).T
  qn = np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
  cn = np.zeros(ld)
  cn[:n] = np.linalg.norm(c.astype(np.float64), axis=1)
  sn = np.repeat(cn.reshape(-1, 128).max(axis=1), 128)[None, :]
  err = np.abs(got[:, :n] - exact)
  bound = qn * sn[:, :n] * 0.00104
  worst = float((err / bound).max())
  print(f"d={d} {data} {mfma}: max |s16 - s| / (||q|| N_stage) = {worst * 0.00104:.3e}")
  assert (err <= bound).all(), worst
  assert (got[:, n:] == 0.0).all()                           # the zero padding of the last stage


_NQ = [1, 64, 500, 513, 1024, 1500, 2048, 3000]
_K = [1, 10, 100, 300]
_KINDS = ["gauss", "row_scales", "clustered", "dups", "hot_queries"]


@pytest.mark.parametrize("d", [32, 64, 100, 128])
def test_both_shapes_keep_every_survivor(d):
  """Whole batches against the all-f32 search (TFRS_TOPK_FILTER=f32), in the style of
  tests/test_fuzz_gpu.py::test_scan16f_instantiations_keep_every_survivor: 40 cases per dim that pair every batch size
  with every kind of data (`hot_queries`: every lane of a tile is hot at once, the queue overflows into the drain inside
  check(); `dups` / `clustered`: bursts), k = 1 .. 300, with the statistical threshold plan on and off; every other corpus
  has a row count that is not a multiple of 128 (the row_limit path of the last stage)."""
  from recommenders_amd import _lib
  from recommenders_amd.layers import factorized_top_k as ftk
  rng = np.random.default_rng(900 + d)
  dev = torch.device("cuda", 0)
  bad = []
  for case in range(40):
    n = int(rng.integers(66_000, 260_000))
    n = n // 128 * 128 + (int(rng.integers(1, 128)) if case % 2 == 0 else 0)
    nq = _NQ[case % 8]
    kind = _KINDS[case % 5]
    k = _K[(case // 2) % 4]
    g = torch.Generator(device=dev).manual_seed(int(rng.integers(1 << 30)))
    c = torch.randn((n, d), generator=g, device=dev) / d ** 0.5
    q = torch.randn((nq, d), generator=g, device=dev) / d ** 0.5
    if kind == "row_scales":
      c *= torch.exp(1.5 * torch.randn((n, 1), generator=g, device=dev))
    elif kind == "clustered":
      cen = torch.randn((32, d), generator=g, device=dev) / d ** 0.5
      c = cen[torch.arange(n, device=dev) * 32 // n] + 0.2 * c
      q = cen[torch.randint(0, 32, (nq,), generator=g, device=dev)] + 0.2 * q
    elif kind == "dups":
      c[n // 3:2 * (n // 3)] = c[:n // 3].clone()
    elif kind == "hot_queries":
      q[:] = q[0]
    layer = ftk.BruteForce(k=k, dedup=(kind != "dups") and "auto").index(c)
    _lib.set_option("TFRS_TOPK_FILTER", "f32")
    try:
      s32, i32 = layer(q)
    finally:
      _lib.set_option("TFRS_TOPK_FILTER", None)
    for arm in ARMS:
      for stat in ("0", "1"):
        _lib.set_option("TFRS_SCAN16_MFMA", arm)
        _lib.set_option("TFRS_TOPK_STAT", stat)
        try:
          s, i = layer(q)
        finally:
          _lib.set_option("TFRS_SCAN16_MFMA", None)
          _lib.set_option("TFRS_TOPK_STAT", None)
        if not (torch.equal(s, s32) and torch.equal(i, i32)):
          bad.append((case, n, k, nq, kind, arm, stat))
  assert not bad, bad


def test_headline_batch_is_the_same_in_both_shapes():
  """The batch bench.py times (BASELINE.json configs[1]: 1 M x 64, 8192 queries, k = 100): both arms return the same
  bits, no query needs the exact redo, and a sample of the queries agrees with the oracle."""
  from recommenders_amd import _lib
  from recommenders_amd.layers import factorized_top_k as ftk
  g = torch.Generator(device="cuda").manual_seed(20261016)
  c = torch.randn((1_000_000, 64), generator=g, device="cuda") / 8
  q = torch.randn((8192, 64), generator=g, device="cuda") / 8
  layer = ftk.BruteForce(k=100).index(c)
  res = {}
  for arm in ARMS:
    _lib.set_option("TFRS_SCAN16_MFMA", arm)
    try:
      res[arm] = layer(q)
      assert layer.last_redo_count() == 0, (arm, layer.last_redo_reasons())
    finally:
      _lib.set_option("TFRS_SCAN16_MFMA", None)
  assert torch.equal(res["32x32"][0], res["16x16"][0]) and torch.equal(res["32x32"][1], res["16x16"][1])
  default = layer(q)
  assert torch.equal(default[0], res["16x16"][0]) and torch.equal(default[1], res["16x16"][1])
  rows = slice(4000, 4064)
  es, ei = o_topk.brute_force(q[rows].cpu().numpy(), c.cpu().numpy(), 100)
  np.testing.assert_array_equal(res["16x16"][1][rows].cpu().numpy(), ei)
  np.testing.assert_array_equal(res["16x16"][0][rows].cpu().numpy(), es)
