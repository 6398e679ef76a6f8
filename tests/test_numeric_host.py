"""Discretization / Normalization without a GPU: exports and constructor errors, the NumPy restatement against
independent implementations (``torch.bucketize``, ``np.searchsorted``, ``np.quantile``), the case in which the f32 rule
and an f64 bucketize disagree, and the argument checks of the C entries."""

import numpy as np
import pytest
import torch

from tests import numeric_restatement as nr


@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


def _layers():
  import recommenders_amd as tfrs
  return tfrs.layers.Discretization, tfrs.layers.Normalization


def test_layers_are_exported():
  import recommenders_amd as tfrs
  from recommenders_amd.layers import numeric
  assert tfrs.layers.Discretization is numeric.Discretization
  assert tfrs.layers.Normalization is numeric.Normalization
  assert callable(numeric.Discretization.adapt)
  for name in ("adapt", "reset_state", "update_state", "finalize_state"):
    assert callable(getattr(numeric.Normalization, name))
  assert numeric.LDS_BOUNDARIES == nr.LDS_BOUNDARIES >= 1000       # the tutorials' 1000 buckets stay in LDS
  assert numeric.MOMENTS_SLICE_ELEMENTS == nr.MOMENTS_SLICE_ELEMENTS
  assert numeric.MOMENTS_MAX_GROUPS == nr.MOMENTS_MAX_GROUPS


def test_header_constants_match_the_python_side():
  import os
  import re
  from recommenders_amd.layers import numeric
  header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tfrs_hip.h")).read()
  value = lambda name: re.search(r"#define %s (\S+)" % name, header).group(1)
  assert int(value("TFRS_BUCKETIZE_LDS_BOUNDARIES")) == numeric.LDS_BOUNDARIES
  assert int(value("TFRS_MOMENTS_SLICE_ELEMENTS")) == numeric.MOMENTS_SLICE_ELEMENTS
  assert int(value("TFRS_MOMENTS_MAX_GROUPS")) == numeric.MOMENTS_MAX_GROUPS
  assert float(value("TFRS_NORMALIZE_EPSILON").rstrip("f")) == numeric.EPSILON
  codes = [int(value("TFRS_NUMERIC_" + n)) for n in ("F32", "F64", "I32", "I64")]
  assert codes == [numeric._DTYPE_CODES[t] for t in (torch.float32, torch.float64, torch.int32, torch.int64)]


def test_discretization_constructor_errors():
  Discretization, _ = _layers()
  with pytest.raises(ValueError, match="sorted"):
    Discretization(bin_boundaries=[0.0, 2.0, 1.0])
  with pytest.raises(ValueError, match="NaN"):
    Discretization(bin_boundaries=[0.0, float("nan")])
  with pytest.raises(NotImplementedError, match="one_hot"):
    Discretization(bin_boundaries=[0.0], output_mode="one_hot")
  for mode in ("multi_hot", "count"):
    with pytest.raises(NotImplementedError):
      Discretization(bin_boundaries=[0.0], output_mode=mode)
  with pytest.raises(NotImplementedError, match="sparse"):
    Discretization(bin_boundaries=[0.0], sparse=True)
  with pytest.raises(ValueError, match="not both"):
    Discretization(bin_boundaries=[0.0], num_bins=4)
  with pytest.raises(ValueError, match="one of"):
    Discretization()
  with pytest.raises(ValueError, match="num_bins"):
    Discretization(num_bins=0)
  layer = Discretization(num_bins=4, epsilon=0.5)           # epsilon is accepted and ignored
  with pytest.raises(RuntimeError, match="adapt"):
    layer(torch.zeros(3))
  assert layer.state_dict().keys() == set()                  # no boundaries yet


def test_normalization_constructor_errors():
  _, Normalization = _layers()
  for axis in (0, 1, -2, (0, 1)):
    with pytest.raises(NotImplementedError, match="axis"):
      Normalization(axis=axis)
  with pytest.raises(ValueError, match="together"):
    Normalization(mean=1.0)
  with pytest.raises(ValueError, match="together"):
    Normalization(axis=None, variance=2.0)
  with pytest.raises(ValueError, match="broadcast"):
    Normalization(mean=[1.0, 2.0], variance=[1.0, 2.0, 3.0])
  with pytest.raises(ValueError, match="scalar"):
    Normalization(axis=None, mean=[1.0, 2.0], variance=[1.0, 2.0])
  with pytest.raises(ValueError, match="last axis"):
    Normalization(mean=np.zeros((2, 3)), variance=np.ones((2, 3)))
  for layer in (Normalization(), Normalization(axis=None), Normalization(axis=(-1,), invert=True)):
    with pytest.raises(RuntimeError, match="statistics"):
      layer(torch.zeros(3))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_layers_fail_loudly_without_gpu():
  Discretization, Normalization = _layers()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    Discretization(bin_boundaries=[0.0, 1.0])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    Discretization(num_bins=4).adapt(torch.arange(10.0))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    Normalization(axis=None, mean=0.0, variance=1.0)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    Normalization().adapt(torch.zeros(4, 3))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    Normalization(axis=None).update_state(np.arange(5))


# ---- the restatement against independent implementations ---------------------------------------------------------
EDGE_BOUNDARIES = np.array([-np.inf, -3.5, -0.0, 0.0, 1.0, 2.0, 2.0, 2.0, 7.25, 1e30, np.inf], dtype=np.float32)


def _edge_values(b):
  finite = b[np.isfinite(b)]
  vals = np.concatenate([b, np.nextafter(finite, np.float32(-np.inf)), np.nextafter(finite, np.float32(np.inf)),
                         np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -1e38, 1e38], np.float32)])
  return vals.astype(np.float32)


def test_restated_bucketize_against_searchsorted_and_torch():
  b = EDGE_BOUNDARIES
  assert (b[5] == b[6] == b[7]) and b[2] == b[3] and np.signbit(b[2]) and not np.signbit(b[3])
  x = _edge_values(b)
  got = nr.bucketize_by_definition(x, b)
  np.testing.assert_array_equal(got, nr.bucketize(x, b))
  np.testing.assert_array_equal(got, np.searchsorted(b, x, side="right"))          # NumPy sorts NaN last: bucket nb
  np.testing.assert_array_equal(got, torch.bucketize(torch.from_numpy(x), torch.from_numpy(b), right=True).numpy())
  assert got[np.isnan(x)].tolist() == [b.size]
  assert nr.bucketize(np.array([2.0], np.float32), b).tolist() == [8]              # past the run of three
  assert nr.bucketize(np.array([-0.0, 0.0], np.float32), b).tolist() == [4, 4]     # -0 == +0: both past both zeros
  assert nr.bucketize(np.array([np.inf, -np.inf], np.float32), b).tolist() == [11, 1]
  x64 = x.astype(np.float64)
  np.testing.assert_array_equal(nr.bucketize(x64, b), np.searchsorted(b.astype(np.float64), x64, side="right"))
  assert nr.bucketize(x, np.empty(0, np.float32)).tolist() == [0] * x.size         # nb = 0, NaN included
  rng = np.random.default_rng(3)
  rb = np.sort(rng.normal(size=257).astype(np.float32))
  rx = rng.normal(size=1000).astype(np.float32)
  np.testing.assert_array_equal(nr.bucketize_by_definition(rx, rb), np.searchsorted(rb, rx, side="right"))
  np.testing.assert_array_equal(nr.bucketize_by_definition(rx.astype(np.float64), rb), nr.bucketize(rx.astype(np.float64), rb))
  ri = rng.integers(-3, 4, size=100)
  np.testing.assert_array_equal(nr.bucketize_by_definition(ri, rb),
                                np.searchsorted(rb, ri.astype(np.float32), side="right"))
  np.testing.assert_array_equal(nr.bucketize_by_definition(ri, rb), nr.bucketize(ri, rb))
  np.testing.assert_array_equal(nr.bucketize(ri.astype(np.int32), rb), nr.bucketize(ri, rb))


def test_f32_rule_differs_from_an_f64_bucketize():
  ts, b = nr.timestamp_case()
  f32_rule, f64_rule = nr.bucketize_by_definition(ts, b), nr.bucketize_f64(ts, b)
  np.testing.assert_array_equal(f32_rule, nr.bucketize(ts, b))
  differ = np.nonzero(f32_rule != f64_rule)[0]
  assert differ.size >= 1, "the GPU test of this input would not tell the two rules apart"
  assert np.abs(f32_rule - f64_rule).max() == 1 and differ.size < ts.size // 100
  # the disagreement is the rounding of the timestamp onto (or across) a boundary
  for i in differ[:8]:
    assert np.float32(ts[i]) != ts[i]
  # ties to even: 2^24 + 1 rounds DOWN onto the boundary 2^24 (same bucket under both rules), 2^24 + 3 rounds UP onto
  # the boundary 2^24 + 4, which it is below in f64
  edge = np.array([2.0 ** 24, 2.0 ** 24 + 4], dtype=np.float32)
  x = np.array([(1 << 24) + 1, (1 << 24) + 3], dtype=np.int64)
  assert x.astype(np.float32).tolist() == edge.tolist()
  assert nr.bucketize(x, edge).tolist() == [1, 2] and nr.bucketize_f64(x, edge).tolist() == [1, 1]


def test_restated_quantiles_against_numpy():
  rng = np.random.default_rng(5)
  for n, bins in ((64, 4), (1000, 8), (1000, 16), (17, 2), (5, 4), (1, 4), (3, 1)):
    v = rng.normal(size=n).astype(np.float32)
    v[: n // 3] = v[0]                                       # ties
    got = nr.quantile_boundaries(v, bins)
    assert got.shape == (bins - 1,) and got.dtype == np.float32
    if bins > 1:                                             # bins are powers of two: i / bins is exact in binary
      want = np.quantile(v, [i / bins for i in range(1, bins)], method="inverted_cdf")
      np.testing.assert_array_equal(got, want.astype(np.float32))
    for i, bound in enumerate(got, start=1):                 # the definition
      assert (v <= bound).sum() * bins >= i * n
      below = v[v < bound]
      assert below.size == 0 or (v <= below.max()).sum() * bins < i * n
  assert nr.quantile_boundaries(np.arange(10), 5).tolist() == [1.0, 3.0, 5.0, 7.0]


def test_restated_normalize_and_moments():
  x = np.array([[1, 2], [3, 6], [5, 10]], dtype=np.int64)
  mean, var = nr.moments(x)
  assert mean.tolist() == [3.0, 6.0] and var.tolist() == [np.float32(8 / 3), np.float32(32 / 3)]
  m1, v1 = nr.moments(x, axis_none=True)
  assert m1.tolist() == [4.5] and v1.tolist() == [np.float32(np.var(x))]
  np.testing.assert_array_equal(nr.normalize(x, mean, var),
                                ((x.astype(np.float32) - mean) / np.sqrt(var)).astype(np.float32))
  assert nr.scale_of([0.0, 1e-20, 4.0]).tolist() == [np.float32(1e-7), np.float32(1e-7), 2.0]
  assert nr.normalize([5.0], [5.0], [0.0]).tolist() == [0.0]
  assert nr.normalize([6.0], [5.0], [0.0]).tolist() == [np.float32(1.0) / np.float32(1e-7)]
  assert nr.denormalize_f64([2.0], [1.0], [9.0]).tolist() == [7.0]
  assert nr.normalize_grad([3.0], [4.0]).tolist() == [1.5] and nr.normalize_grad([3.0], [4.0], True).tolist() == [6.0]
  assert nr.ulp_distance([1.0, -0.0], [np.nextafter(np.float32(1), np.float32(2)), 0.0]).tolist() == [1, 0]
  # the offset case of unix seconds: f32 tf.nn.moments-style arithmetic is far off, which is why the kernels use f64
  k = np.random.default_rng(7).integers(0, 1000, size=1 << 16)
  ts = 893_000_000 + 64 * k
  mean, var = nr.moments(ts, axis_none=True)
  naive_mean, naive_var = nr.moments_f32_naive(ts)
  assert nr.ulp_distance(var, naive_var)[0] > 1                       # (NumPy's pairwise sums: the mild form of it)
  assert var[0] == np.float32(np.var((64 * k).astype(np.float64)))     # 893e6 + 64 k is an f32 value: exact shift


# ---- the C entries' argument checks (before any HIP call) ------------------------------------------------------------
def test_c_entries_reject_bad_arguments(lib):
  from recommenders_amd import _lib
  E, OK = _lib.TFRS_EINVAL, _lib.TFRS_OK
  buf = np.zeros(64, dtype=np.float64)       # host memory: never dereferenced, the checks come first
  p = buf.ctypes.data
  assert lib.tfrs_bucketize(None, 0, 4, p, 2, p, None) == E and "NULL" in _lib.last_error()
  assert lib.tfrs_bucketize(p, 0, 4, p, 2, None, None) == E
  assert lib.tfrs_bucketize(p, 0, 4, None, 2, p, None) == E and "boundaries" in _lib.last_error()
  assert lib.tfrs_bucketize(p, 0, -1, p, 2, p, None) == E and "count" in _lib.last_error()
  assert lib.tfrs_bucketize(p, 0, 4, p, -1, p, None) == E
  for code in (-1, 4, 99):
    assert lib.tfrs_bucketize(p, code, 4, p, 2, p, None) == E and "dtype" in _lib.last_error()
  assert lib.tfrs_bucketize(p + 4, 1, 4, p, 2, p, None) == E and "aligned" in _lib.last_error()   # f64 at 4 bytes
  assert lib.tfrs_bucketize(None, 0, 0, None, 0, None, None) == OK                                  # n == 0
  assert lib.tfrs_bucketize(None, 3, 0, p, 1000, None, None) == OK

  norm = lambda x, dtype, rows, f, mean, scale, mode, out: lib.tfrs_normalize(x, dtype, rows, f, mean, scale, mode,
                                                                              out, None)
  assert norm(None, 0, 4, 1, p, p, 0, p) == E and "NULL" in _lib.last_error()
  assert norm(p, 0, 4, 1, p, p, 0, None) == E
  assert norm(p, 0, 4, 1, None, p, 0, p) == E and norm(p, 0, 4, 1, p, None, 0, p) == E
  assert norm(p, 0, -1, 1, p, p, 0, p) == E and norm(p, 0, 4, 0, p, p, 0, p) == E and norm(p, 0, 4, -3, p, p, 0, p) == E
  assert norm(p, 7, 4, 1, p, p, 0, p) == E and "dtype" in _lib.last_error()
  assert norm(p, 0, 4, 1, p, p, 4, p) == E and "mode" in _lib.last_error()
  assert norm(p, 0, 4, 1, p, p, -1, p) == E
  assert norm(None, 0, 0, 3, p, p, 0, None) == OK

  size = lib.tfrs_moments_workspace_bytes
  upd = lambda x, dtype, rows, f, state, ws, nbytes: lib.tfrs_moments_update(x, dtype, rows, f, state, ws, nbytes, None)
  assert upd(None, 0, 4, 1, p, p, size(4, 1)) == E and "NULL" in _lib.last_error()
  assert upd(p, 0, 4, 1, None, p, size(4, 1)) == E
  assert upd(p, 0, 4, 1, p, None, size(4, 1)) == E
  assert upd(p, 0, -4, 1, p, p, 1 << 20) == E and upd(p, 0, 4, 0, p, p, 1 << 20) == E
  assert upd(p, 9, 4, 1, p, p, 1 << 20) == E and "dtype" in _lib.last_error()
  assert upd(p, 0, 4, 1, p, p, size(4, 1) - 1) == E and "workspace" in _lib.last_error()
  assert upd(p, 0, 3 * nr.MOMENTS_SLICE_ELEMENTS, 1, p, p, size(2 * nr.MOMENTS_SLICE_ELEMENTS, 1)) == E
  assert upd(None, 0, 0, 5, p, None, 0) == OK                      # an empty batch is a no-op
  assert lib.tfrs_moments_finalize(None, 1, p, p, p, None) == E and "NULL" in _lib.last_error()
  assert lib.tfrs_moments_finalize(p, 1, p, p, None, None) == E
  assert lib.tfrs_moments_finalize(p, 0, p, p, p, None) == E
  assert lib.tfrs_moments_reset(None, 1, None) == E and lib.tfrs_moments_reset(p, 0, None) == E
  with pytest.raises(ValueError, match="bucketize"):
    _lib.check(lib.tfrs_bucketize(p, 12, 4, p, 2, p, None))


def test_moments_workspace_is_positive_and_monotone(lib):
  size = lib.tfrs_moments_workspace_bytes
  rows = [0, 1, 2, 63, 4095, 4096, 4097, 8192, 8193, 100_000, 1 << 20, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 1 << 30,
          1 << 40, 1 << 62]
  feats = [1, 2, 3, 13, 64, 65, 200, 255, 256, 257, 4096, 4097, 10_000]
  table = np.array([[size(n, f) for f in feats] for n in rows], dtype=object)
  assert all(v > 0 for v in table.reshape(-1))
  assert all(table[i + 1, j] >= table[i, j] for i in range(len(rows) - 1) for j in range(len(feats)))
  assert all(table[i, j + 1] >= table[i, j] for i in range(len(rows)) for j in range(len(feats) - 1))
  # what the second launch reads: one (count, mean, M2) triple per workgroup and feature
  for n, f in ((1, 1), (4097, 1), (10, 13), (1000, 13), (1 << 22, 3)):
    groups = -(-n // nr.moments_slice_rows(n, f))
    assert size(n, f) >= groups * f * 24
  assert size(1 << 62, 13) == nr.MOMENTS_MAX_GROUPS * 13 * 24
