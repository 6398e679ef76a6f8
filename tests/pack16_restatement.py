"""NumPy restatement of the fp16 prefilter image, written from the layout and constants that csrc/common.h DOCUMENTS
("fp16 prefilter image": StageMeta, padded_dim16, row_bytes16, pow2_ceil), not from the packing kernels:

  * the corpus is cut into stages of 128 rows; stage s stores x / scale_s with scale_s = pow2_ceil(max |x| of the stage);
  * image row r holds padded_dim16(d) halves in natural feature order -- float16(x / scale), round to nearest even,
    fp16 subnormals kept, zero columns from d on -- followed by one zero 16-byte slot: row_bytes16 = 2 * dp16 + 16;
  * rows at and beyond n (up to the next stage boundary) are zero;
  * the norms the filter's bound is built from must be upper bounds of the float64 row norms computed here.

Host only (no GPU, no library): tests/test_pack16_host.py pins it on cases written out by hand,
tests/test_pack16_layout_gpu.py compares every packing kernel with it bit for bit."""

import numpy as np

STAGE_ROWS = 128                      # kTileN
KAPPA = float(np.float32(0.0011))     # kF16Kappa as the kernels hold it
NORM_SLACK = float(np.float32(1.0002))  # kNormSlack
TINY = 1.0e-30                        # kF16Tiny


def padded_dim16(d: int) -> int:
  for dp in (16, 32, 64, 128):
    if d <= dp:
      return dp
  raise ValueError(f"dim {d} > 128")


def row_bytes16(dp16: int) -> int:
  return dp16 * 2 + 16


def pow2_ceil(x) -> np.ndarray:
  """Smallest power of two >= x for finite x > 0, clamped to [2^-120, 2^120]; 1 for x == 0 (and for non-finite x)."""
  x = np.asarray(x, dtype=np.float32)
  out = np.ones(x.shape, dtype=np.float64)
  ok = np.isfinite(x) & (x > 0)
  m, e = np.frexp(x[ok].astype(np.float64))          # x = m * 2^e, 0.5 <= m < 1 (exact, subnormal floats included)
  e = np.where(m == 0.5, e - 1, e)
  out[ok] = np.ldexp(1.0, np.clip(e, -120, 120))
  return out.astype(np.float32)


def n_stages(n: int) -> int:
  return (n + STAGE_ROWS - 1) // STAGE_ROWS


def _padded(c: np.ndarray) -> np.ndarray:
  c = np.asarray(c, dtype=np.float32)
  out = np.zeros((n_stages(c.shape[0]) * STAGE_ROWS, c.shape[1]), dtype=np.float32)
  out[:c.shape[0]] = c
  return out


def stage_scales(c: np.ndarray) -> np.ndarray:
  """float32 [stages]: pow2_ceil of the stage's largest |x| (1 for an all-zero stage)."""
  p = _padded(c)
  return pow2_ceil(np.abs(p).reshape(-1, STAGE_ROWS * p.shape[1]).max(axis=1))


def image_bytes(c: np.ndarray) -> np.ndarray:
  """uint8 [stages * 128, row_bytes16]: the expected image, little-endian halves."""
  p = _padded(c)
  d = p.shape[1]
  dp16 = padded_dim16(d)
  scale = np.repeat(stage_scales(c).astype(np.float64), STAGE_ROWS)[:, None]
  halves = np.zeros((p.shape[0], dp16 + 8), dtype="<f2")          # + 8 halves = the 16-byte pad slot
  halves[:, :d] = (p.astype(np.float64) / scale).astype(np.float16)   # exact quotient, ONE rounding (nearest even)
  return halves.view(np.uint8).reshape(p.shape[0], row_bytes16(dp16))


def true_row_norms(c: np.ndarray) -> np.ndarray:
  """float64 [n]: the 2-norm of every row, from float64 squares (no under- or overflow for any float32 row)."""
  return np.linalg.norm(np.asarray(c, dtype=np.float32).astype(np.float64), axis=1)


def true_stage_norms(c: np.ndarray) -> np.ndarray:
  """float64 [stages]: the largest true row norm of every stage."""
  n = np.zeros(n_stages(np.shape(c)[0]) * STAGE_ROWS)
  n[:np.shape(c)[0]] = true_row_norms(c)
  return n.reshape(-1, STAGE_ROWS).max(axis=1)
