"""The inputs of the fp16 prefilter's bound, read back from the device (csrc/common.h, "fp16 prefilter image"):

    |s16 - s| <= qk[q] * meta.norm[stage(row)] + kF16Tiny

The filter kernels subtract qk * norm from their threshold and the list kernel keeps a band of 2 * (qk * norm_max + tiny),
so the top-K is exact only while the COMPUTED norms are upper bounds of the true ones.  These tests read the fp16 image,
StageMeta and norm_max through tfrs_debug_fp16_image, and qk / qscale from the scratch buffer of tfrs_debug_fp16_scores,
and hold them to tests/pack16_restatement.py (bit for bit where the value is determined, as an upper bound within a
derived factor where it is a norm) -- at ordinary magnitudes and at both ends of the float32 range, where a plain f32
sum of squares under- or overflows.  Nothing here times anything."""

import ctypes

import numpy as np
import pytest

from oracle import topk as o_topk
from tests import pack16_restatement as rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ARMS = ["32x32", "16x16"]
# kNormSlack = 1.0002 on top of an f32 sum of at most 128 squares (128 * 2^-24 = 7.7e-6) and one square root
NORM_FACTOR = 1.0003


@pytest.fixture(params=ARMS)
def mfma(request):
  from recommenders_amd import _lib
  _lib.set_option("TFRS_SCAN16_MFMA", request.param)
  yield request.param
  _lib.set_option("TFRS_SCAN16_MFMA", None)


def _ftk():
  from recommenders_amd.layers import factorized_top_k
  return factorized_top_k


def _np(x):
  return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _read_image(handle, n, d):
  """(image uint8 [stages * 128, row_bytes16], meta float32 [stages, 4], norm_max float32) of the whole index."""
  from recommenders_amd import _lib
  stages = rs.n_stages(n)
  rb = rs.row_bytes16(rs.padded_dim16(d))
  img = torch.full((stages * 128 * rb,), 0xA5, dtype=torch.uint8, device="cuda")
  meta = torch.full((stages, 4), float("nan"), dtype=torch.float32, device="cuda")
  nmax = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
  _lib.check(_lib.load().tfrs_debug_fp16_image(handle.handle, 0, stages, _lib.ptr(img), _lib.ptr(meta), _lib.ptr(nmax),
                                               _lib.current_stream()))
  return _np(img).reshape(stages * 128, rb), _np(meta), _np(nmax)[0]


def _scores_and_query_side(handle, q_dev, nq, n):
  """tfrs_debug_fp16_scores over rows [0, n): (scores float64 [nq, n], qk float32 [nq], qscale float32 [nq])."""
  from recommenders_amd import _lib
  ld = rs.n_stages(n) * 128
  out = torch.full((nq, ld), float("nan"), dtype=torch.float32, device="cuda")
  scratch = torch.full((2 * nq,), float("nan"), dtype=torch.float32, device="cuda")
  _lib.check(_lib.load().tfrs_debug_fp16_scores(handle.handle, ctypes.c_void_p(q_dev.data_ptr()), nq, 0, n, _lib.ptr(out),
                                                _lib.ptr(scratch), _lib.current_stream()))
  s = _np(scratch)
  return _np(out)[:, :n].astype(np.float64), s[:nq], s[nq:]


def _row_scale_data(rng, n, d, nq=0):
  """The data of tests/test_topk_gpu.py::test_f16_prefilter_error_bound: row norms spread by e^(3 N(0, 1)), elements
  1e-5 of their neighbours inside rows."""
  c = (rng.normal(size=(n, d)) * np.exp(rng.normal(size=(n, 1)) * 3.0)).astype(np.float32)
  c[:, ::3] *= np.float32(1e-5)
  q = (rng.normal(size=(nq, d)) * np.exp(rng.normal(size=(nq, 1)))).astype(np.float32)
  q[:, 1::4] *= np.float32(3e-6)
  return c, q


def _assert_image_and_meta(c, img, meta, nmax, tight=True):
  """Image and scales bit for bit; norms as upper bounds (within NORM_FACTOR when `tight`); norm_max = max norm."""
  np.testing.assert_array_equal(img, rs.image_bytes(c))
  scale = rs.stage_scales(c)
  np.testing.assert_array_equal(meta[:, 1].view(np.uint32), scale.view(np.uint32))
  np.testing.assert_array_equal(meta[:, 2].view(np.uint32), (np.float32(1.0) / scale).view(np.uint32))
  assert not meta[:, 3].any()
  true = rs.true_stage_norms(c)
  norm = meta[:, 0].astype(np.float64)
  assert (true <= norm).all(), (true, norm)
  if tight:
    assert (norm <= true * NORM_FACTOR).all(), (norm / np.maximum(true, 1e-300)).max()
  assert nmax.view(np.uint32) == meta[:, 0].max().view(np.uint32), (nmax, meta[:, 0].max())


# ---- image and metadata, every packer -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1317])
@pytest.mark.parametrize("d", [1, 5, 8, 9, 16, 17, 32, 33, 48, 64, 65, 100, 128])
def test_image_scales_and_norms_of_every_packer(d, n):
  """pack16_stage_kernel (d <= 8) and pack16_stage_regs_kernel<16 | 32 | 64 | 128> (zero-padded dims in between), one
  row to ten stages and a bit: fewer than 65536 rows are not shuffled, image row = candidate row."""
  c, _ = _row_scale_data(np.random.default_rng(1000 * d + n), n, d)
  layer = _ftk().BruteForce(k=1).index(c)
  _assert_image_and_meta(c, *_read_image(layer._index, n, d))


@pytest.mark.parametrize("d", [5, 64])
def test_all_zero_stage(d):
  """Stage 1 of three is all zero: scale 1, norm 0, zero image; its neighbours are untouched by it."""
  c, _ = _row_scale_data(np.random.default_rng(d), 300, d)
  c[128:256] = 0.0
  img, meta, nmax = _read_image(_ftk().BruteForce(k=1).index(c)._index, 300, d)
  assert meta[1].tolist() == [0.0, 1.0, 1.0, 0.0]
  assert not img[128:256].any()
  _assert_image_and_meta(c, img, meta, nmax)
  # ... and a corpus that is all zero
  z = np.zeros((130, d), dtype=np.float32)
  img, meta, nmax = _read_image(_ftk().BruteForce(k=1).index(z)._index, 130, d)
  assert not img.any() and nmax == 0.0 and meta.tolist() == [[0.0, 1.0, 1.0, 0.0]] * 2


# ---- ingest paths ---------------------------------------------------------------------------------------------------
_BLOCKS = [37, 91, 128, 1, 300, 129, 90, 256, 285]     # ends at 37, 128 (fills a stage), 256 (a whole stage), 257, ...


@pytest.mark.parametrize("d", [5, 48, 128])
def test_ingest_paths_build_the_same_image(d):
  """index() on the whole array, index_from_dataset(total_rows=n) over blocks, and reserve + one append per block
  (blocks that straddle, end on and exactly fill stages -- a partly filled tail stage is rebuilt by the next append)
  leave the same image, meta and norm_max, bit for bit."""
  from recommenders_amd import _lib
  from recommenders_amd.layers.factorized_top_k._common import _IndexHandle
  n = 1317
  assert sum(_BLOCKS) == n
  c, _ = _row_scale_data(np.random.default_rng(31 + d), n, d)
  # the largest rows first: norm_max is reached in the first block and must survive the later appends
  c = c[np.argsort(-rs.true_row_norms(c), kind="stable")]
  whole = _read_image(_ftk().BruteForce(k=1).index(c)._index, n, d)
  _assert_image_and_meta(c, *whole)
  cuts = np.cumsum([0] + _BLOCKS)
  dev = [torch.as_tensor(c[a:b]).cuda() for a, b in zip(cuts[:-1], cuts[1:])]
  from_ds = _read_image(_ftk().BruteForce(k=1).index_from_dataset(dev, total_rows=n)._index, n, d)
  handle = _IndexHandle()
  lib = _lib.load()
  _lib.check(lib.tfrs_index_reserve(handle.handle, n, d, _lib.current_stream()))
  for blk in dev:
    _lib.check(lib.tfrs_index_append(handle.handle, _lib.ptr(blk), blk.shape[0], _lib.current_stream()))
  appended = _read_image(handle, n, d)
  for other in (from_ds, appended):
    np.testing.assert_array_equal(other[0], whole[0])
    np.testing.assert_array_equal(other[1].view(np.uint32), whole[1].view(np.uint32))
    assert other[2].view(np.uint32) == whole[2].view(np.uint32)


@pytest.mark.parametrize("d", [5, 64])
def test_reindex_forgets_the_previous_norm_max(d):
  """The same layer, and the same library handle, re-indexed with a corpus of 1e-3 times the norms: norm_max is the new
  corpus's, not the stale larger one (it is accumulated with an atomic max, so it has to be zeroed)."""
  from recommenders_amd import _lib
  from recommenders_amd.layers.factorized_top_k._common import _IndexHandle
  n = 700
  c, _ = _row_scale_data(np.random.default_rng(77 + d), n, d)
  small = (c * np.float32(2.0 ** -10)).astype(np.float32)       # (a power of two: the image is the same, the scales move)
  layer = _ftk().BruteForce(k=1)
  big_max = _read_image(layer.index(c)._index, n, d)[2]
  img, meta, nmax = _read_image(layer.index(small)._index, n, d)
  _assert_image_and_meta(small, img, meta, nmax)
  assert nmax.view(np.uint32) == (big_max * np.float32(2.0 ** -10)).view(np.uint32)
  handle = _IndexHandle()
  lib = _lib.load()
  for corpus in (c, small):
    t = torch.as_tensor(corpus).cuda()
    _lib.check(lib.tfrs_index_set(handle.handle, _lib.ptr(t), n, d, _lib.current_stream()))
    _assert_image_and_meta(corpus, *_read_image(handle, n, d))


# ---- query side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("nq", [5, 16, 17, 203])
@pytest.mark.parametrize("d", [1, 5, 16, 63, 64, 100, 128])
def test_query_scale_and_kappa(d, nq, offset):
  """query_kappa_kernel: 16 lanes per query, 16 queries per 256-thread workgroup -- 5 leave it partly full, 16 fill it,
  17 and 203 spill into further ones.  A query pointer 4 bytes off a 16-byte boundary (and every d that is no multiple
  of 4) takes the kernel's scalar branch.  Query 2 is zero; the last two are scaled to the ends of the float32 range,
  where a plain sum of squares is 0 or Inf."""
  _, q = _row_scale_data(np.random.default_rng(5000 + 10 * d + nq), 1, d, nq)
  q[2] = 0.0
  q[nq - 2] = q[nq - 2] * np.float32(2.0 ** -100)
  q[nq - 1] = q[nq - 1] * np.float32(2.0 ** 100)
  q[nq - 1, 0] = np.float32(2.0 ** 100)                         # (never all zero, whatever d)
  q[nq - 2, 0] = np.float32(2.0 ** -100)
  c = np.ones((128, d), dtype=np.float32)
  layer = _ftk().BruteForce(k=1).index(c)
  buf = torch.zeros((nq * d + 4,), dtype=torch.float32, device="cuda")
  assert buf.data_ptr() % 16 == 0
  q_dev = buf[offset:offset + nq * d]
  q_dev.copy_(torch.as_tensor(q.reshape(-1)))
  _, qk, qscale = _scores_and_query_side(layer._index, q_dev, nq, 128)
  np.testing.assert_array_equal(qscale.view(np.uint32), rs.pow2_ceil(np.abs(q).max(axis=1)).view(np.uint32))
  qn = np.linalg.norm(q.astype(np.float64), axis=1)
  qk = qk.astype(np.float64)
  assert (qn * rs.KAPPA <= qk).all(), (qn * rs.KAPPA, qk)
  mid = np.ones(nq, dtype=bool)
  mid[[nq - 2, nq - 1]] = False                                 # (outside [2^-60, 2^60] the bound may be sqrt(d) loose)
  assert (qk[mid] <= qn[mid] * rs.KAPPA * NORM_FACTOR).all(), (qk[mid] / np.maximum(qn[mid] * rs.KAPPA, 1e-300)).max()
  assert (qk[~mid] <= qn[~mid] * rs.KAPPA * NORM_FACTOR * np.sqrt(d)).all()
  assert qk[2] == 0.0 and qscale[2] == 1.0


# ---- the invariant itself, across the float32 range --------------------------------------------------------------
_E = [-100, -80, -70, -40, 0, 40, 58]        # corpus x 2^e
_F = [-80, -40, 0, 20]                       # queries x 2^f
# |e + f| <= 90 keeps ||q|| ||c|| (2^(e + f) times a factor of 2^-15 .. 2^25 for this data) inside the normal f32 range
_PAIRS = [(e, f) for e in _E for f in _F if abs(e + f) <= 90]


def _assert_invariant(layer, c, q, tag):
  n, nq = c.shape[0], q.shape[0]
  img, meta, nmax = _read_image(layer._index, n, c.shape[1])
  s16, qk, _ = _scores_and_query_side(layer._index, torch.as_tensor(q).cuda(), nq, n)
  true = rs.true_stage_norms(c)
  norm = meta[:, 0].astype(np.float64)
  qn = np.linalg.norm(q.astype(np.float64), axis=1)
  nz = true > 0
  lo, hi = (norm[nz] / true[nz]).min(), (norm[nz] / true[nz]).max()
  print(f"NORM_RATIO {tag} d={c.shape[1]}: meta.norm / true norm in [{lo:.6f}, {hi:.6f}], "
        f"qk / (||q|| kappa) in [{(qk / (qn * rs.KAPPA)).min():.6f}, {(qk / (qn * rs.KAPPA)).max():.6f}]")
  bad = []
  if not (true <= norm).all():
    bad.append(f"meta.norm below the true norm: ratio {lo:.3e}")
  if not (qn * rs.KAPPA <= qk.astype(np.float64)).all():
    bad.append(f"qk below ||q|| kappa: ratio {(qk / (qn * rs.KAPPA)).min():.3e}")
  if nmax.view(np.uint32) != meta[:, 0].max().view(np.uint32):
    bad.append("norm_max is not the largest stage norm")
  exact = q.astype(np.float64) @ c.astype(np.float64).T
  rhs = qk.astype(np.float64)[:, None] * np.repeat(norm, 128)[None, :n] + rs.TINY   # what the filter subtracts
  err = np.abs(s16 - exact)
  if not (err <= rhs).all():
    bad.append(f"|s16 - s| exceeds qk * meta.norm + tiny by up to {(err / rhs).max():.3e} x "
               f"({int((err > rhs).sum())} of {err.size} pairs)")
  return [f"{tag}: {b}" for b in bad]


@pytest.mark.parametrize("d", [32, 64, 100])
def test_bound_from_the_device_holds_across_the_f32_range(d, mfma):
  """For every (query, row): |s16 - s_float64| <= qk[q] * meta.norm[stage(row)] + 1e-30 with the right side AS THE
  DEVICE HOLDS IT, the corpus scaled by 2^e and the queries by 2^f (powers of two: the image and the prefilter scores are
  the same up to the scale, the norms are not -- their squares leave the f32 range from 2^-63 / 2^64 on).  1317 rows
  (the last stage holds 37), 203 queries (the last group of 32 holds 11)."""
  n, nq = 1317, 203
  c0, q0 = _row_scale_data(np.random.default_rng(800 + d), n, d, nq)
  bad = []
  for e in _E:
    c = (c0 * np.float32(2.0 ** e)).astype(np.float32)
    layer = _ftk().BruteForce(k=10).index(c)
    for f in [f for (ee, f) in _PAIRS if ee == e]:
      q = (q0 * np.float32(2.0 ** f)).astype(np.float32)
      bad += _assert_invariant(layer, c, q, f"{mfma} corpus x 2^{e} queries x 2^{f}")
  assert not bad, "\n".join(bad)


@pytest.mark.parametrize("d", [32, 64, 100])
def test_bound_holds_for_a_unit_row_among_tiny_ones(d, mfma):
  """One row of norm 1 among rows of norm 1e-28: its stage must carry the unit row's norm, every other stage a bound
  of rows whose squares are all zero in f32."""
  n, nq = 1317, 203
  rng = np.random.default_rng(900 + d)
  c = rng.normal(size=(n, d))
  c = c / np.linalg.norm(c, axis=1, keepdims=True) * 1e-28
  c[5] *= 1e28
  c = c.astype(np.float32)
  q = (rng.normal(size=(nq, d)) / np.sqrt(d)).astype(np.float32)
  bad = _assert_invariant(_ftk().BruteForce(k=10).index(c), c, q, f"{mfma} unit row among 1e-28 rows")
  assert not bad, "\n".join(bad)


# ---- searches are exact at the edges -----------------------------------------------------------------------------
_EDGE = ["corpus_x1e-23", "corpus_x1e-24", "queries_x1e-24", "corpus_x2^58", "row_of_1e19"]
_EDGE_CACHE = {}


def _edge_case(setting, n, k):
  """The clustered corpus (66048 x 64; rows 5000 .. 5599 are one direction with 3e-4 relative noise per element; 32 of
  the 64 queries are aligned with it) in one of the settings, its first n rows, and the oracle's top-k: computed once
  per (setting, n, k) and shared, never modified."""
  key = (setting, n, k)
  if key not in _EDGE_CACHE:
    rng = np.random.default_rng(20261020)
    N, d, nq = 66048, 64, 64
    c = (rng.normal(size=(N, d)) / 8).astype(np.float32)
    base = (rng.normal(size=(1, d)) / 8).astype(np.float32)
    c[5000:5600] = (base * (1.0 + 3e-4 * rng.normal(size=(600, d)))).astype(np.float32)
    q = (rng.normal(size=(nq, d)) / 8).astype(np.float32)
    q[:32] = base * rng.uniform(1.0, 4.0, size=(32, 1)).astype(np.float32)
    if setting == "corpus_x1e-23":
      c = c * np.float32(1e-23)
    elif setting == "corpus_x1e-24":
      c = c * np.float32(1e-24)
    elif setting == "queries_x1e-24":
      q = q * np.float32(1e-24)
    elif setting == "corpus_x2^58":
      c = c * np.float32(2.0 ** 58)
    elif setting == "row_of_1e19":
      # every element finite and below 1.8e19, yet the row's SQUARED norm (6.4e39) is beyond float32; one zero query
      c[777] = np.float32(1e19)
      q[40] = 0.0
    c = np.ascontiguousarray(c[:n], dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    assert np.isfinite(c).all() and np.isfinite(q).all()
    es, ei = o_topk.brute_force(q, c, k)
    _EDGE_CACHE[key] = (c, q, es, ei)
  return _EDGE_CACHE[key]


def _plan(n, k, shuffled):
  from recommenders_amd import _lib
  plan = (ctypes.c_int64 * 5)()
  _lib.check(_lib.load().tfrs_debug_topk_plan(n, k, shuffled, plan))
  return list(plan)


@pytest.mark.parametrize("setting", _EDGE)
def test_bruteforce_default_is_exact_at_the_edges(setting, mfma):
  """BruteForce(k=100) on 66048 rows, default settings: the shuffled index, threshold from sampled stages."""
  n, k = 66048, 100
  c, q, es, ei = _edge_case(setting, n, k)
  assert _plan(n, k, 1)[1] > 0                       # sampled stages: the fp16 path runs
  s, i = _ftk().BruteForce(k=k).index(c)(q)
  np.testing.assert_array_equal(_np(i), ei)
  np.testing.assert_array_equal(_np(s), es)


@pytest.mark.parametrize("setting", _EDGE)
def test_bruteforce_eager_is_exact_at_the_edges(setting, mfma, monkeypatch):
  """BruteForce(k=10) on 8320 rows under the "f16-eager" settings of tests/test_topk_gpu.py (threshold pass over all
  stages of an index that is not shuffled)."""
  monkeypatch.setenv("TFRS_TOPK_FILTER", "f16")
  monkeypatch.setenv("TFRS_TOPK_MINBINS", "1")
  monkeypatch.setenv("TFRS_TOPK_SAMPLE", "1")
  n, k = 8320, 10
  c, q, es, ei = _edge_case(setting, n, k)
  assert _plan(n, k, 0)[1] > 0                       # sampled stages: the fp16 path really runs at this size
  s, i = _ftk().BruteForce(k=k).index(c)(q)
  np.testing.assert_array_equal(_np(i), ei)
  np.testing.assert_array_equal(_np(s), es)


class _LazyBlocks:
  """A dataset that yields fresh device tensors on every pass (never cached: the blocks are searched in place)."""

  def __init__(self, c, rows):
    self.c, self.rows = c, rows

  def __iter__(self):
    for lo in range(0, self.c.shape[0], self.rows):
      yield torch.as_tensor(self.c[lo:lo + self.rows]).cuda()


@pytest.mark.parametrize("regime", ["raw16", "f16"])
@pytest.mark.parametrize("setting", _EDGE)
def test_streaming_is_exact_at_the_edges(setting, regime, mfma, monkeypatch):
  """Streaming over blocks read in place, with the switches of
  tests/test_topk_gpu.py::test_streaming_groups_read_blocks_in_place: "raw16" = the fp16 filter fed by the f32 blocks
  (norms per 16 / 32 rows inside the scan kernels), "f16" = the group's fp16 image built from the blocks
  (pack16_raw_kernel).  Blocks of 2048 rows = 16 stages, the smallest that take the fp16 path."""
  if regime == "raw16":
    monkeypatch.setenv("TFRS_STREAM_RAW16_MIN_NQ", "1")
  else:
    monkeypatch.setenv("TFRS_STREAM_RAW16_MAX_NQ", "0")
    monkeypatch.setenv("TFRS_STREAM_RAW_MAX_NQ", "0")
    monkeypatch.setenv("TFRS_STREAM_RHO16", "2")
  n, k = 66048, 100
  c, q, es, ei = _edge_case(setting, n, k)
  layer = _ftk().Streaming(k=k).index_from_dataset(_LazyBlocks(c, 2048))
  s, i = layer(q)
  assert layer._cache is None
  np.testing.assert_array_equal(_np(i), ei)
  np.testing.assert_array_equal(_np(s), es)
