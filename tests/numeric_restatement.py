"""NumPy restatement of the numeric preprocessing kernels (``csrc/numeric.hip``): bucketize under the f32 rule,
normalize in f32, the two-pass f64 moments of the f32 values, and the inverted-CDF quantiles of ``adapt``."""

import numpy as np

F32 = np.float32
LDS_BOUNDARIES = 4095            # TFRS_BUCKETIZE_LDS_BOUNDARIES
ELEMENTWISE_GRID_PASS = {4: 2048 * 256 * 4, 8: 2048 * 256 * 2}   # elements one pass of the capped grid covers, by itemsize
MOMENTS_SLICE_ELEMENTS = 4096    # TFRS_MOMENTS_SLICE_ELEMENTS
MOMENTS_MAX_GROUPS = 1024        # TFRS_MOMENTS_MAX_GROUPS
EPSILON = F32(1e-7)


def _compared(x, boundaries):
  x = np.asarray(x)
  b = np.asarray(boundaries, dtype=F32).reshape(-1)
  if x.dtype == np.float64:
    return x, b.astype(np.float64)
  assert x.dtype in (np.float32, np.int32, np.int64), x.dtype
  return x.astype(F32), b


def bucketize_by_definition(x, boundaries) -> np.ndarray:
  """out[i] = #{ j : boundaries[j] <= x[i] } with f32 boundaries.  f32, int32 and int64 input is compared in f32
  (integers rounded to nearest even by ``astype``); f64 input in f64 against the widened boundaries.  NaN -> nb."""
  xc, bc = _compared(x, boundaries)
  out = np.zeros(xc.shape, dtype=np.int64)
  for v in bc:                       # the definition itself, not a search
    out += (v <= xc)
  out[np.isnan(xc)] = bc.size
  return out


def bucketize(x, boundaries) -> np.ndarray:
  """The same by binary search (NumPy orders NaN after +inf, which is bucket nb): the form the large cases use."""
  xc, bc = _compared(x, boundaries)
  return np.searchsorted(bc, xc, side="right").astype(np.int64)


def bucketize_f64(x, boundaries) -> np.ndarray:
  """What an all-f64 comparison would give: differs from ``bucketize`` where an integer is no f32 value."""
  return np.searchsorted(np.asarray(boundaries, dtype=F32).astype(np.float64), np.asarray(x).astype(np.float64),
                         side="right")


def scale_of(variance) -> np.ndarray:
  with np.errstate(invalid="ignore"):
    return np.maximum(np.sqrt(np.asarray(variance, dtype=F32)), EPSILON).astype(F32)


def normalize(x, mean, variance) -> np.ndarray:
  """(f32(x) - mean) / scale, every operation rounded to f32."""
  x32 = np.asarray(x).astype(F32)
  with np.errstate(all="ignore"):
    return ((x32 - np.asarray(mean, F32)).astype(F32) / scale_of(variance)).astype(F32)


def denormalize_f64(x, mean, variance) -> np.ndarray:
  """f32(x) * scale + mean in f64, rounded to f32 once more: within one f32 ulp of a fused multiply-add."""
  x64 = np.asarray(x).astype(F32).astype(np.float64)
  with np.errstate(all="ignore"):
    return (x64 * scale_of(variance).astype(np.float64) + np.asarray(mean, F32).astype(np.float64)).astype(F32)


def normalize_grad(g, variance, invert=False) -> np.ndarray:
  g32, s = np.asarray(g, F32), scale_of(variance)
  return (g32 * s if invert else g32 / s).astype(F32)


def moments(x, axis_none=False):
  """(mean, variance) of the f32-converted values, two passes in f64, rounded to f32 at the end; per last-axis
  feature unless ``axis_none``."""
  x64 = np.asarray(x).astype(F32).astype(np.float64)
  x64 = x64.reshape(-1, 1) if axis_none else x64.reshape(-1, x64.shape[-1])
  mean = x64.mean(axis=0)
  var = ((x64 - mean) ** 2).mean(axis=0)
  return mean.astype(F32), var.astype(F32)


def moments_f32_naive(x):
  """tf.nn.moments-style f32 arithmetic (f32 mean, f32 mean of squared differences): what the issue measures against."""
  x32 = np.asarray(x).astype(F32).reshape(-1)
  mean = x32.mean(dtype=F32)
  return mean, ((x32 - mean) ** 2).mean(dtype=F32)


def quantile_boundaries(values, num_bins: int) -> np.ndarray:
  """Boundary i (1 <= i < num_bins): the smallest value v with at least i n / num_bins of the n f32 values <= v."""
  v = np.sort(np.asarray(values).astype(F32).reshape(-1))
  n = v.size
  ranks = [-(-i * n // num_bins) for i in range(1, num_bins)]      # ceil, in integers
  return v[[max(r, 1) - 1 for r in ranks]] if ranks else np.empty((0,), F32)


def ulp_distance(a, b) -> np.ndarray:
  """Distance in f32 ulps between arrays of finite f32 values (ordered-integer form of the bit patterns)."""
  def ordered(x):
    i = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)
  return np.abs(ordered(a) - ordered(b))


def moments_slice_rows(n_rows: int, f: int) -> int:
  base = max(1, -(-MOMENTS_SLICE_ELEMENTS // f))
  return max(base, -(-n_rows // MOMENTS_MAX_GROUPS))


def timestamp_case(seed=11, n=4096):
  """int64 unix seconds of the MovieLens range against the tutorials' 1000 ``linspace`` buckets."""
  rng = np.random.default_rng(seed)
  ts = rng.integers(875_000_000, 893_000_000, size=n, endpoint=True)
  ts[:2] = [875_000_000, 893_000_000]
  return ts, np.linspace(ts.min(), ts.max(), 1000).astype(F32)
