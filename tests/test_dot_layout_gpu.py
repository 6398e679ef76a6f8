"""The DotInteraction kernels (csrc/interaction.hip: nine kernels behind one decision function) on the hand-built inputs
of tests/dot_handbuilt.py, through the C entry points, so that no Python dispatch chooses the path.  The inputs are exact
under every route (tests/test_dot_handbuilt_host.py proves it from the arrays, and that the cases reach every (kernel,
template arguments) the decision function can choose): every output is compared with the float64 result as values,
with no tolerance.

Every output lies between two runs of sentinels that must survive and is pre-filled with a NaN pattern, so an element
nobody wrote shows; for the strided entries the prefix columns and the gap right of the pairs are sentinels too."""

import numpy as np
import pytest

from tests import dot_handbuilt as hb
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 192                       # floats of sentinel on both sides of every output: longer than the longest triangle row (129)
SENTINEL = -0x38383839            # int32 0xC7C7C7C7: the float -102343.555
UNWRITTEN = 0x7FC0DEAD            # a quiet NaN nobody computes
GATE_DOT = {"fwd": 1.6e-6, "bwd": 1.2e-6}     # tests/test_ops_gpu.py: the ceilings of this operation


def _lib():
  from recommenders_amd import _lib as L
  return L, L.load()


def _dev(a, off=0):
  """The array on the device, ``off`` bytes past a 16-byte boundary of a fresh allocation."""
  a = np.ascontiguousarray(a, np.float32)
  buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
  v = buf[off // 4: off // 4 + a.size]
  v.copy_(torch.from_numpy(a.reshape(-1)))
  assert a.size == 0 or v.data_ptr() % 16 == off
  return v


class _Out:
  """``size`` floats of the NaN pattern between two runs of sentinels, ``off`` bytes past a 16-byte boundary."""

  def __init__(self, size, off=0):
    self.lo, self.size = GUARD + off // 4, int(size)
    self.raw = torch.full((self.lo + self.size + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    self.raw[self.lo: self.lo + self.size] = UNWRITTEN
    self.t = self.raw.view(torch.float32)[self.lo: self.lo + self.size]
    assert self.size == 0 or self.t.data_ptr() % 16 == off

  def guards_intact(self, tag):
    assert bool((self.raw[: self.lo] == SENTINEL).all()) and bool((self.raw[self.lo + self.size:] == SENTINEL).all()), \
        f"{tag}: a sentinel next to the output was overwritten"

  def untouched(self, tag):
    self.guards_intact(tag)
    assert bool((self.raw[self.lo: self.lo + self.size] == UNWRITTEN).all()), f"{tag}: a refused call wrote to its output"

  def check(self, tag, ref):
    """Equal to the float64 reference as values (0.0 == -0.0; an unwritten element is a NaN and differs)."""
    self.guards_intact(tag)
    want = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, np.float64).reshape(-1)).cuda()
    got = self.t.double()
    if not torch.equal(got, want.reshape(-1).double()):
      bad = torch.nonzero(~(got == want.reshape(-1).double())).reshape(-1)
      first = [(int(i), float(got[i]), float(want.reshape(-1)[i])) for i in bad[:6]]
      raise AssertionError(f"{tag}: {bad.numel()} of {self.size} entries differ; (flat index, got, want): {first}")


def _p(t):
  L, _ = _lib()
  return L.ptr(t.t if isinstance(t, _Out) else t)


def _run(case, x, dy, off_x=0, off_out=0):
  """Both entry points on the case's shape under its switches: (out, dx) as _Out."""
  L, lib = _lib()
  s = L.current_stream()
  b, f, d = case.batch, case.f, case.d
  with hb.switches(*case.sw):
    xd, dyd = _dev(x, off_x), _dev(dy, off_out)
    out, dx = _Out(b * case.n, off_out), _Out(b * f * d, off_x)
    rc = lib.tfrs_dot_interaction_fwd(_p(xd), b, f, d, case.self_i, case.skip, _p(out), s)
    if case.planned()["fwd"]["kernel"] == hb.REFUSED:    # (two backward routes exist only where the forward is refused)
      assert rc == L.TFRS_ENOTIMPL
      torch.cuda.synchronize()
      out.untouched(f"{case} refused forward")
      out = None
    else:
      L.check(rc)
    L.check(lib.tfrs_dot_interaction_bwd(_p(xd), _p(dyd), b, f, d, case.self_i, case.skip, _p(dx), s))
    torch.cuda.synchronize()
  return out, dx


def _exact(case, off_x=0, off_out=0):
  c = case.build()
  out, dx = _run(case, c["x"], c["dy"], off_x, off_out)
  dx.check(f"{case} backward", c["dx"])
  if out is None:
    return
  out.check(f"{case} forward", c["out"])
  p = hb.planted(case.batch, case.f)
  n, fd = case.n, case.f * case.d
  assert not out.t[p["zero_x"] * n: (p["zero_x"] + 1) * n].any()
  assert not dx.t[p["zero_x"] * fd: (p["zero_x"] + 1) * fd].any() and not dx.t[p["zero_dy"] * fd: (p["zero_dy"] + 1) * fd].any()


# ------------------------------------------------------------------------------------------ every route
@pytest.mark.parametrize("case", hb.ROUTE_CASES, ids=str)
def test_route(case):
  """One case per (kernel, template arguments) the decision function can choose (and the MAXE, dense-tile and
  16-byte-load edges of the backward), forward and backward, F just inside its row block, d = DP and d < DP."""
  _exact(case)


@pytest.mark.parametrize("case,off_x,off_out", hb.ALIGNMENT, ids=str)
def test_alignment(case, off_x, off_out):
  """x and dx off a 16-byte boundary (the scalar loads), out and dout off an 8-byte boundary, odd and even out_dim
  (the float2 or the dword copy-out of the staged kernels), F * d not a multiple of 4."""
  _exact(case, off_x, off_out)


@pytest.mark.parametrize("route,f,d,self_i,sw", hb.GRID_STRIDE, ids=str)
def test_grid_stride_and_prefetch(route, f, d, self_i, sw):
  """The persistent kernels at batch = 2 * stride + 5 (stride: the samples of one trip of the grid): the second trip of
  the sample loop, the fetch of the next sample under the copy-out, and a last trip that only five waves make.  (The
  reference of these larger batches is float64 on the device; numpy for the small skip_gather case.)"""
  case, stride = hb.grid_stride_case(route, f, d, self_i, sw)
  assert case.batch == 2 * stride + 5
  c = hb.build(case.batch, f, d, self_i, case.skip, hb.case_rng("stride", route, sorted(sw.items())))
  out, dx = _run(case, c["x"], c["dy"])
  if case.skip:
    out.check(f"{case} forward", c["out"])
    dx.check(f"{case} backward", c["dx"])
    return
  x64, dy64 = torch.from_numpy(c["x"]).cuda().double(), torch.from_numpy(c["dy"]).cuda().double()
  g = torch.einsum("bik,bjk->bij", x64, x64)
  r, cidx = (torch.from_numpy(v).cuda() for v in hb.packed_index(f, self_i))
  out.check(f"{case} forward", g[:, r, cidx])
  low = torch.zeros((case.batch, f, f), dtype=torch.float64, device="cuda")
  low[:, r, cidx] = dy64
  dx.check(f"{case} backward", torch.einsum("bij,bjk->bik", low + low.transpose(1, 2), x64))
  assert bool(torch.equal(g[:, r, cidx], torch.from_numpy(c["out"]).cuda()))         # the two references agree


# ------------------------------------------------------------------------------------------ the strided entries
@pytest.mark.parametrize("prefix", hb.STRIDED_PREFIX)
@pytest.mark.parametrize("case", hb.STRIDED, ids=str)
def test_strided_equals_contiguous(case, prefix):
  """The pairs as columns prefix .. prefix + pairs - 1 of a [batch, prefix + pairs + 5] matrix: bit for bit what the
  contiguous call returns, the prefix columns and the gap right of the pairs untouched; the backward reads its
  gradient from such a matrix whose other columns hold NaNs."""
  L, lib = _lib()
  s = L.current_stream()
  b, f, d, n = case.batch, case.f, case.d, case.n
  assert lib.tfrs_dot_interaction_strided_supported(b, f, d, case.self_i) == 1
  c = case.build()
  flat = hb.Case(case.route, b, f, d, case.self_i)
  out, dx = _run(flat, c["x"], c["dy"])
  out.check(f"{case} contiguous forward", c["out"])
  dx.check(f"{case} contiguous backward", c["dx"])
  width = prefix + n + 5
  wide = _Out(b * width)
  rows = wide.raw[wide.lo: wide.lo + b * width].view(b, width)
  rows[:] = SENTINEL
  rows[:, prefix: prefix + n] = UNWRITTEN
  xd = _dev(c["x"])
  grad = torch.full((b, width), float("nan"), dtype=torch.float32, device="cuda")
  grad[:, prefix: prefix + n] = torch.from_numpy(c["dy"]).cuda()
  dxs = _Out(b * f * d)
  L.check(lib.tfrs_dot_interaction_fwd_strided(_p(xd), b, f, d, case.self_i, wide.t.data_ptr() + 4 * prefix, width, s))
  L.check(lib.tfrs_dot_interaction_bwd_strided(_p(xd), grad.data_ptr() + 4 * prefix, width, b, f, d, case.self_i, _p(dxs), s))
  torch.cuda.synchronize()
  wide.guards_intact(f"{case} strided forward")
  assert bool((rows[:, :prefix] == SENTINEL).all()) and bool((rows[:, prefix + n:] == SENTINEL).all()), \
      f"{case}: the strided forward wrote outside its columns"
  assert torch.equal(rows[:, prefix: prefix + n].reshape(-1), out.t.view(torch.int32))
  dxs.guards_intact(f"{case} strided backward")
  assert torch.equal(dxs.t.view(torch.int32), dx.t.view(torch.int32))


# ------------------------------------------------------------------------------------------ refused shapes, no pairs
@pytest.mark.parametrize("shape", hb.REFUSED_CASES, ids=str)
def test_refused_shapes_write_nothing(shape):
  L, lib = _lib()
  s = L.current_stream()
  b, f, d, self_i, skip = shape
  n = hb.out_dim(f, self_i, skip)
  x = _dev(np.ones((b, f, d), np.float32))
  out = _Out(b * n)
  assert lib.tfrs_dot_interaction_fwd(_p(x), b, f, d, self_i, skip, _p(out), s) == L.TFRS_ENOTIMPL
  assert f"{f} features x {d} dims" in L.last_error()
  torch.cuda.synchronize()
  out.untouched(f"forward {shape}")
  if not skip:
    wide = _Out(b * (n + 5))
    assert lib.tfrs_dot_interaction_fwd_strided(_p(x), b, f, d, self_i, _p(wide), n + 5, s) == L.TFRS_ENOTIMPL
    assert "strided" in L.last_error()
    torch.cuda.synchronize()
    wide.untouched(f"strided forward {shape}")
  from recommenders_amd.layers.feature_interaction import DotInteraction
  feats = [torch.ones((b, d), device="cuda") for _ in range(f)]
  result = None
  with pytest.raises(NotImplementedError):
    result = DotInteraction(self_interaction=bool(self_i), skip_gather=bool(skip))(feats)
  assert result is None


def test_backward_refuses_past_its_envelope():
  L, lib = _lib()
  b, f, d = 5, 140, 130
  x, dy, dx = _dev(np.ones((b, f, d), np.float32)), _dev(np.ones((b, hb.pairs(f, 0)), np.float32)), _Out(b * f * d)
  assert lib.tfrs_dot_interaction_bwd(_p(x), _p(dy), b, f, d, 0, 0, _p(dx), L.current_stream()) == L.TFRS_ENOTIMPL
  assert "140 features x 130 dims" in L.last_error()
  torch.cuda.synchronize()
  dx.untouched("backward 140 x 130")


def test_one_feature_without_self_interaction():
  """No pairs: an empty [B, 0] output and a zero gradient of shape [B, 1, D], through the layer (whose empty tensors
  have NULL data pointers) and through the entry points, which launch nothing."""
  from recommenders_amd.layers.feature_interaction import DotInteraction
  L, lib = _lib()
  b, d = 67, 8
  x = torch.randn((b, d), device="cuda", requires_grad=True)
  out = DotInteraction()([x])
  assert out.shape == (b, 0) and out.dtype == torch.float32
  out.backward(torch.empty((b, 0), device="cuda"))
  assert x.grad.shape == (b, d) and not x.grad.any()
  xd, dx = _dev(np.ones((b, 1, d), np.float32)), _Out(b * d)
  L.check(lib.tfrs_dot_interaction_fwd(_p(xd), b, 1, d, 0, 0, None, L.current_stream()))
  L.check(lib.tfrs_dot_interaction_bwd(_p(xd), None, b, 1, d, 0, 0, _p(dx), L.current_stream()))
  torch.cuda.synchronize()
  dx.check("one feature, backward", np.zeros(b * d))
  # with self interaction and with skip_gather the single feature has an output
  for self_i, skip in ((1, 0), (0, 1), (1, 1)):
    _exact(hb.Case("fwd.any", b, 1, d, self_i, skip))


# ------------------------------------------------------------------------------------------ rounding, once per route
@pytest.mark.parametrize("case", hb.ROUNDING, ids=str)
def test_rounding(case):
  """N(0, 1) inputs times a per-sample exp(4 N(0, 1)) scale against the float64 oracle, relative to the sum of |terms|
  of every entry, under the ceilings the project has for this operation."""
  from oracle import feature_interaction as o_fi
  x, dy = hb.rounding_inputs(case.batch, case.f, case.d, case.self_i, case.skip, hb.case_rng("rounding", case.id))
  plan = case.planned()
  out, dx = _run(case, x, dy)
  dx.guards_intact(f"{case} backward")
  feats = [x[:, j, :] for j in range(case.f)]
  yf, yb = o_fi.dot_interaction_yardsticks(feats, dy, case.self_i, case.skip)
  got_b = dx.t.cpu().numpy().reshape(yb.shape)
  assert np.isfinite(got_b).all() and not got_b[1].any() and not got_b[3].any()
  ef = None
  if out is not None:                                                    # (None: a backward route whose forward is refused)
    out.guards_intact(f"{case} forward")
    got_f = out.t.cpu().numpy().reshape(yf.shape)
    assert np.isfinite(got_f).all() and not got_f[1].any()
    ef = float_gate(f"dot_layout.{hb.route_name('fwd', plan['fwd'])[4:]}.fwd", got_f, hb.forward64(x, case.self_i, case.skip),
                    yf, GATE_DOT["fwd"])
  eb = float_gate(f"dot_layout.{hb.route_name('bwd', plan['bwd'])[4:]}.bwd", got_b, hb.backward64(x, dy, case.self_i, case.skip),
                  yb, GATE_DOT["bwd"])
  print(f"{case}: forward {ef}, backward {eb:.3e}")
