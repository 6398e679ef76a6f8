"""tests/pack16_restatement.py on cases small enough to write out by hand (no GPU, no library): the GPU tests of
tests/test_pack16_layout_gpu.py compare the packing kernels with this restatement bit for bit, so the restatement
itself is pinned here against literal bytes."""

import numpy as np

from tests import pack16_restatement as rs


def test_pow2_ceil_at_its_edges():
  one = np.float32(1.0)
  got = rs.pow2_ceil(np.array([0.0, 1.0, np.nextafter(one, np.float32(2.0)), 2.0 ** -130, 2.0 ** 125], dtype=np.float32))
  assert got.dtype == np.float32
  assert got.tolist() == [1.0, 1.0, 2.0, 2.0 ** -120, 2.0 ** 120]
  # ... and between them: exact powers map to themselves, everything else to the next one; non-finite -> 1
  got = rs.pow2_ceil(np.array([0.5, 0.75, 3.0, 4.0, 2.0 ** -120, 2.0 ** -149, 2.0 ** 120, 3.0e38, np.inf, np.nan],
                              dtype=np.float32))
  assert got.tolist() == [0.5, 1.0, 4.0, 4.0, 2.0 ** -120, 2.0 ** -120, 2.0 ** 120, 2.0 ** 120, 1.0, 1.0]


def test_two_row_stage_byte_for_byte():
  """d = 3, two rows: max |x| = 3 -> scale 4.  Row 0 / 4 = (0.25, -0.125, 0.0625); row 1 / 4 = (0.75, 2^-24: the
  smallest fp16 SUBNORMAL, 2^-14: the smallest fp16 normal).  dp16 = 16: 32 bytes of halves + the 16-byte pad slot."""
  c = np.array([[1.0, -0.5, 0.25],
                [3.0, 2.0 ** -22, 2.0 ** -12]], dtype=np.float32)
  assert rs.padded_dim16(3) == 16 and rs.row_bytes16(16) == 48
  assert rs.stage_scales(c).tolist() == [4.0]
  img = rs.image_bytes(c)
  assert img.shape == (128, 48) and img.dtype == np.uint8
  row0 = [0x00, 0x34, 0x00, 0xB0, 0x00, 0x2C] + [0] * 42       # 0x3400, 0xB000, 0x2C00 little-endian
  row1 = [0x00, 0x3A, 0x01, 0x00, 0x00, 0x04] + [0] * 42       # 0x3A00, 0x0001, 0x0400
  assert img[0].tolist() == row0
  assert img[1].tolist() == row1
  assert not img[2:].any()                                     # rows at and beyond n
  np.testing.assert_array_equal(rs.true_row_norms(c), [np.sqrt(1.0 + 0.25 + 0.0625),
                                                       np.sqrt(9.0 + 2.0 ** -44 + 2.0 ** -24)])
  assert rs.true_stage_norms(c).tolist() == [np.sqrt(9.0 + 2.0 ** -44 + 2.0 ** -24)]


def test_rounding_is_to_nearest_even_and_stages_scale_apart():
  """1 + 2^-11 lies halfway between two halves and goes to the even one (1.0); 1 + 3 * 2^-11 goes up to 1 + 2^-9
  (even significand).  Values below 2^-25 of the scale vanish.  The second stage (rows 128 ..) has its own scale, an
  all-zero third stage has scale 1."""
  c = np.zeros((300, 2), dtype=np.float32)
  c[0] = (1.0, 1.0 + 2.0 ** -11)        # stage max 1 + 2^-11 -> scale 2: halves of 0.5, 0.5 + 2^-12 -> 0.5 (tie, even)
  c[1] = (1.0 + 3 * 2.0 ** -11, 2.0 ** -26)   # / 2 = 0.5 + 3 * 2^-12: tie between 0.5 + 2^-11 and 0.5 + 2^-10 -> even
  c[128] = (-2.0 ** -100, 2.0 ** -101)  # scale 2^-100: -1.0 and 0.5
  assert rs.stage_scales(c).tolist() == [2.0, 2.0 ** -100, 1.0]
  img = rs.image_bytes(c).view("<u2")
  assert img[0, :2].tolist() == [0x3800, 0x3800]
  assert img[1, :2].tolist() == [0x3802, 0x0000]
  assert img[128, :2].tolist() == [0xBC00, 0x3800]
  assert not img[256:].any()
  # float64 norms neither underflow nor overflow where float32 squares do
  tiny = np.full((1, 64), 1e-30, dtype=np.float32)
  huge = np.full((1, 64), 1e19, dtype=np.float32)
  np.testing.assert_allclose(rs.true_row_norms(tiny), [8.0 * float(np.float32(1e-30))], rtol=1e-15)
  np.testing.assert_allclose(rs.true_row_norms(huge), [8.0 * float(np.float32(1e19))], rtol=1e-15)
