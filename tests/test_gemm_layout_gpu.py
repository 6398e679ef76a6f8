"""The GEMM kernels (csrc/gemm16.hip: the row / column operand preparation in every variant, both tile kernels, split-K and
its reduction, ``g16_mul_kernel``; csrc/interaction.hip: ``gemm_kernel`` in every transposition with its split-K,
the column sums, ``act_pointwise_bwd_kernel``) on the hand-built operands of tests/gemm_handbuilt.py, through the C
entry points, so that no Python dispatch chooses the path.  Both families are exact in float32 in any summation order
(tests/test_gemm_handbuilt_host.py proves it from the arrays, and that the cases reach every variant the planner can
choose): every output is compared with the float64 result BIT FOR BIT.

Every call gets a workspace filled with 0xFF bytes (NaN in both float widths: a read of an image cell or a partial
product nobody wrote shows up), every output lies inside a larger buffer of sentinels that must survive, and operands
are views 4, 8 and 12 bytes into their storage where the plan says that changes the path."""

import contextlib

import numpy as np
import pytest

from tests import gemm_handbuilt as hb

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64                        # floats of sentinel on both sides of every output
SENTINEL = -0x38383839            # int32 0xC7C7C7C7: the float -102343.555


def _ids(v):
  return str(v).replace(" ", "")


def _lib():
  from recommenders_amd import _lib as L
  return L, L.load()


@contextlib.contextmanager
def _tile(tile):
  L, _ = _lib()
  try:
    L.set_option("TFRS_GEMM16_TILE", str(tile) if tile else None)
    yield
  finally:
    L.set_option("TFRS_GEMM16_TILE", None)


def _dev(a, off=0):
  """The array on the device, ``off`` bytes into a fresh allocation (None stays None)."""
  if a is None:
    return None
  a = np.ascontiguousarray(a, np.float32)
  buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
  v = buf[off // 4: off // 4 + a.size]
  v.copy_(torch.from_numpy(a.reshape(-1)))
  assert v.data_ptr() % 16 == off
  return v


_WANT = {}                        # id(reference) -> (reference, its float32 copy on the device), per test


@pytest.fixture(autouse=True)
def _forget_references():
  _WANT.clear()
  yield
  _WANT.clear()


def _want(ref):
  if id(ref) not in _WANT:
    assert ref.size > (1 << 20) or hb.exact_f32(ref)      # (the host test proves it for the large ones)
    _WANT[id(ref)] = (ref, torch.from_numpy(np.ascontiguousarray(ref.astype(np.float32)).reshape(-1)).cuda())
  return _WANT[id(ref)][1]


class _Out:
  """An output of ``size`` floats between two runs of sentinels (``off`` bytes past a 16-byte boundary)."""

  def __init__(self, size, off=0, init=None):
    self.lo, self.size = GUARD + off // 4, int(size)
    self.raw = torch.full((self.lo + self.size + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    self.t = self.raw.view(torch.float32)[self.lo: self.lo + self.size]
    if init is not None:
      self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, np.float32).reshape(-1)))

  def check(self, tag, ref):
    assert bool((self.raw[: self.lo] == SENTINEL).all()) and bool((self.raw[self.lo + self.size:] == SENTINEL).all()), \
        f"{tag}: a sentinel next to the output was overwritten"
    if not torch.equal(self.t, _want(ref)):
      got, w = self.t.cpu().numpy().reshape(ref.shape), ref.astype(np.float32)
      bad = np.argwhere(~((got == w) | (np.isnan(got) & np.isnan(w))))
      first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(w[tuple(i)])) for i in bad[:6]]
      raise AssertionError(f"{tag}: {len(bad)} of {ref.size} entries differ; (index, got, want): {first}")
    return self.t.clone()


def _ws(nbytes):
  return torch.full((int(nbytes) + 256,), 0xFF, dtype=torch.uint8, device="cuda"), int(nbytes)


def _p(t):
  L, _ = _lib()
  return L.ptr(t if not isinstance(t, _Out) else t.t)


def _rng(*key):
  return hb.case_rng(*key)


# ------------------------------------------------------------------------------------------ split-fp16: q c^T
@pytest.mark.parametrize("family", ["int", "sel_a", "sel_b"])
@pytest.mark.parametrize("case", hb.SCORES16, ids=_ids)
def test_scores_f16(case, family):
  """tfrs_compute_scores, f16: both operands go through the ROW preparation (B is read as [n, k]) -- every variant of
  the K-step-major prep under the 256-tile kernel, the row-per-wave prep under the 128-tile kernel, split-K with
  ragged tiles, a short last slice and every tail of the reduction."""
  m, n, k, tile, offa, offb = case
  L, lib = _lib()
  c = hb.product(family, m, n, k, _rng("scores16", family, case), tile)
  with _tile(tile):
    q, cand = _dev(c["a"], offa), _dev(c["b"].T, offb)
    ws, nb = _ws(lib.tfrs_gemm_f16_workspace_bytes(m, n, k))
    first = None
    for run in range(2 if tile == 0 else 1):
      out = _Out(m * n)
      ws.fill_(0xFF)
      L.check(lib.tfrs_compute_scores(_p(q), _p(cand), m, n, k, _p(out), 1, _p(ws), nb, L.current_stream()))
      got = out.check(f"scores16 {family} {case}", c["ref"])
      assert first is None or torch.equal(first.view(torch.int32), got.view(torch.int32))
      first = got


# ------------------------------------------------------------------------------------------ split-fp16: Dense forward
@pytest.mark.parametrize("case,family", [(c, f) for c in hb.DENSE_FWD16 for f in ("int", "sel_a", "sel_b")
                                         if f == "int" or not (c[4] or c[5])], ids=_ids)
def test_dense_fwd_f16(case, family):
  """tfrs_dense_fwd_f16 / tfrs_dense_fwd_act (f16): B goes through the COLUMN passes (one or many 256-row slabs, both
  image layouts, with and without 16-byte loads); without bias and activation the long-K shapes split."""
  m, n, k, tile, has_bias, act, offb = case
  L, lib = _lib()
  c = hb.product(family, m, n, k, _rng("dense16", family, case), tile)
  bias = hb.small_ints((n,), _rng("bias", case), -50, 50) if has_bias else None
  pre = c["ref"] + (hb.f64(bias) if has_bias else 0.0)
  with _tile(tile):
    x, w, b = _dev(c["a"]), _dev(c["b"], offb), _dev(bias)
    ws, nb = _ws(lib.tfrs_gemm_f16_workspace_bytes(m, n, k))
    pre_out = _Out(m * n)
    if act or has_bias:
      for a_code, want, pre_buf in ((1 if act else 0, hb.relu(pre) if act else pre, pre_out), (0, pre, None)):
        out = _Out(m * n)
        ws.fill_(0xFF)
        L.check(lib.tfrs_dense_fwd_act(_p(x), _p(w), _p(b), m, k, n, a_code, _p(out), _p(pre_buf), 1, _p(ws), nb,
                                       L.current_stream()))
        out.check(f"dense_fwd_act f16 {case}", want)
        if pre_buf is not None:
          pre_buf.check(f"dense_fwd_act f16 pre {case}", pre)
    out = _Out(m * n)
    ws.fill_(0xFF)
    L.check(lib.tfrs_dense_fwd_f16(_p(x), _p(w), _p(b), m, k, n, _p(out), _p(ws), nb, L.current_stream()))
    out.check(f"dense_fwd_f16 {family} {case}", pre)


# ------------------------------------------------------------------------------------------ split-fp16: Cross forward
@pytest.mark.parametrize("case", hb.CROSS_FWD16, ids=_ids)
def test_cross_fwd_f16(case):
  batch, d, tile = case
  L, lib = _lib()
  s = L.current_stream()
  lin = hb.cross_fwd_case(batch, d, _rng("cross16", case), tile)
  act = hb.cross_fwd_case(batch, d, _rng("cross16", case), tile, relu_act=True)
  with _tile(tile):
    x0, x, w, b = _dev(lin["x0"]), _dev(lin["x"]), _dev(lin["w"]), _dev(lin["bias"])
    ws, nb = _ws(lib.tfrs_gemm_f16_workspace_bytes(batch, d, d))
    y = _Out(batch * d)
    L.check(lib.tfrs_cross_fwd_f16(_p(x0), _p(x), _p(w), _p(b), lin["diag"], batch, d, _p(y), _p(ws), nb, s))
    y.check(f"cross_fwd_f16 {case}", lin["y"])
    y, u = _Out(batch * d), _Out(batch * d)
    ws.fill_(0xFF)
    L.check(lib.tfrs_cross_fwd_f16_train(_p(x0), _p(x), _p(w), _p(b), lin["diag"], batch, d, _p(y), _p(u), _p(ws), nb, s))
    y.check(f"cross_fwd_f16_train y {case}", lin["y"])
    u.check(f"cross_fwd_f16_train u {case}", lin["u"])
    for code, c in ((1, act), (0, lin)):
      y, pre = _Out(batch * d), _Out(batch * d)
      ws.fill_(0xFF)
      L.check(lib.tfrs_cross_fwd_act(_p(x0), _p(x), _p(x), d, _p(w), _p(b), c["diag"], code, batch, d, _p(y), _p(pre), 1,
                                     _p(ws), nb, s))
      y.check(f"cross_fwd_act f16 act={code} {case}", c["y"])
      pre.check(f"cross_fwd_act f16 pre act={code} {case}", c["pre"])


# ------------------------------------------------------------------------------------------ split-fp16: Cross backward
def _cross_bwd_variants(L, lib, tag, c, batch, d, offs=(0, 0, 0, 0)):
  """Every f16 Cross backward entry on one case.  offs: byte offsets of (dy, u, dx0, dx0_add)."""
  s = L.current_stream()
  x0, x, w, b = _dev(c["x0"]), _dev(c["x"]), _dev(c["w"]), _dev(c["bias"])
  dy, u = _dev(c["dy"], offs[0]), _dev(c["u"], offs[1])
  ws, nb = _ws(lib.tfrs_cross_bwd_workspace_bytes(batch, d, 1))
  n = batch * d

  def outs(db=True, dx0_init=None):
    return _Out(n, offs[2], dx0_init), _Out(n), _Out(d * d), (_Out(d) if db else None)

  def check(name, o, dx0_ref):
    o[0].check(f"{tag} {name} dx0", dx0_ref)
    o[1].check(f"{tag} {name} dx", c["dx"])
    o[2].check(f"{tag} {name} dkernel", c["dw"])
    if o[3] is not None:
      o[3].check(f"{tag} {name} dbias", c["db"])

  for db in (True, False):
    o = outs(db)
    ws.fill_(0xFF)
    L.check(lib.tfrs_cross_bwd_f16(_p(x0), _p(x), _p(w), _p(b), c["diag"], _p(dy), batch, d, _p(o[0]), _p(o[1]), _p(o[2]),
                                   _p(o[3]), _p(ws), nb, s))
    check(f"cross_bwd_f16 db={db}", o, c["dx0"])
  o = outs()
  ws.fill_(0xFF)
  L.check(lib.tfrs_cross_bwd_f16_saved(_p(x0), _p(x), _p(u), _p(w), c["diag"], _p(dy), batch, d, _p(o[0]), _p(o[1]),
                                       _p(o[2]), _p(o[3]), _p(ws), nb, s))
  check("cross_bwd_f16_saved", o, c["dx0"])
  for add_mode in ("none", "distinct", "alias"):
    for add_dx in (0, 1):
      add = None if add_mode == "none" else c["add"]
      o = outs(dx0_init=add if add_mode == "alias" else None)
      add_t = None if add is None else (o[0].t if add_mode == "alias" else _dev(add, offs[3]))
      ws.fill_(0xFF)
      L.check(lib.tfrs_cross_bwd_f16_saved_acc(_p(x0), _p(x), _p(u), _p(w), c["diag"], _p(dy), batch, d, _p(add_t), add_dx,
                                               _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), _p(ws), nb, s))
      want = c["dx0"] + (0.0 if add is None else hb.f64(add)) + (c["dx"] if add_dx else 0.0)
      check(f"cross_bwd_f16_saved_acc add={add_mode} add_dx={add_dx}", o, want)


@pytest.mark.parametrize("case", hb.CROSS_BWD16, ids=_ids)
def test_cross_bwd_f16(case):
  """The fused multiplier dz = dy * x0 in the row preparation at every k = d of the table (256-tile kernel), in the
  row-per-wave prep (128-tile kernel) and in the column passes of dW = x^T dz, whose A operand goes through the
  column passes too; db from the column-maximum pass; batch >= 8192: dW splits."""
  batch, d, tile = case
  L, lib = _lib()
  c = hb.cross_bwd_case(batch, d, _rng("crossbwd16", case), tile)
  with _tile(tile):
    _cross_bwd_variants(L, lib, f"{case}", c, batch, d)


MUL_OFFSETS = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 12, 0), (0, 0, 0, 4)]


@pytest.mark.parametrize("count,offs", [(c, o) for c in hb.MUL_COUNTS for o in MUL_OFFSETS] +
                         [("big", MUL_OFFSETS[0]), ("big", MUL_OFFSETS[3])], ids=_ids)
def test_mul_kernel_counts_and_alignments(count, offs):
  """g16_mul_kernel (dx0 = dy * u + dx0_add + dx of the saved-u backward): vector body, vector body with a scalar tail,
  the scalar form when any pointer is off a 16-byte boundary, in place, and a second round of its grid-stride loop."""
  batch, d = hb.BIG_MUL if count == "big" else (count, 1)
  L, lib = _lib()
  c = hb.cross_bwd_case(batch, d, _rng("mul", batch, d), 0)
  _cross_bwd_variants(L, lib, f"mul {count} {offs}", c, batch, d, offs)


# ------------------------------------------------------------------------------------------ Dense backward, both GEMMs
def _dense_bwd(L, lib, tag, c, batch, din, dout, f16, offs=(0, 0, 0)):
  s = L.current_stream()
  x, w, dy, add = _dev(c["x"], offs[0]), _dev(c["w"], offs[1]), _dev(c["dy"], offs[2]), _dev(c["add"])
  ws, nb = _ws(lib.tfrs_dense_bwd_workspace_bytes(batch, din, dout, f16))
  for mask in range(8):                                     # every NULL-output combination (0: nothing to do)
    dx = _Out(batch * din) if mask & 1 else None
    dw = _Out(din * dout) if mask & 2 else None
    db = _Out(dout) if mask & 4 and c["db"] is not None else None
    for addend in ((None, add) if add is not None and mask & 1 else (None,)):
      ws.fill_(0xFF)
      if addend is None:
        rc = lib.tfrs_dense_bwd(_p(x), _p(w), _p(dy), batch, din, dout, _p(dx), _p(dw), _p(db), f16, _p(ws), nb, s)
      else:
        rc = lib.tfrs_dense_bwd_add(_p(x), _p(w), _p(dy), _p(addend), batch, din, dout, _p(dx), _p(dw), _p(db), f16,
                                    _p(ws), nb, s)
      L.check(rc)
      name = f"{tag} f16={f16} mask={mask} addend={addend is not None}"
      if dx is not None:
        dx.check(name + " dx", c["dx"] if addend is None else c["dx_add"])
      if dw is not None:
        dw.check(name + " dkernel", c["dw"])
      if db is not None:
        db.check(name + " dbias", c["db"])


@pytest.mark.parametrize("family", ["int", "sel"])
@pytest.mark.parametrize("case", hb.DENSE_BWD16, ids=_ids)
def test_dense_bwd_f16(case, family):
  """dx: rows of dy against W read as [n, k]; dW = x^T dy: BOTH operands through the column passes (A side: colmax_a),
  split at batch >= 8192; db alone: the column-maximum pass and its reduction, no product."""
  batch, din, dout, tile = case
  L, lib = _lib()
  c = hb.dense_bwd_case(family, batch, din, dout, _rng("densebwd16", family, case), tile)
  with _tile(tile):
    _dense_bwd(L, lib, f"{family} {case}", c, batch, din, dout, 1)


@pytest.mark.parametrize("off", hb.BWD32_OFFSETS)
@pytest.mark.parametrize("family", ["int", "sel"])
@pytest.mark.parametrize("case", hb.DENSE_BWD32, ids=_ids)
def test_dense_bwd_f32(case, family, off):
  """The f32 kernel: A^T B with its split-K on both sides of K = 2048, ragged last slices, three and more slices;
  A B^T; the column sums; 16-byte loads on and off by leading dimension and by pointer."""
  batch, din, dout = case
  L, lib = _lib()
  c = hb.dense_bwd_case(family, batch, din, dout, _rng("densebwd32", family, case))
  _dense_bwd(L, lib, f"{family} {case} off={off}", c, batch, din, dout, 0, (off, off, off))


@pytest.mark.parametrize("case", hb.CROSS_BWD32, ids=_ids)
def test_cross_bwd_f32(case):
  """tfrs_cross_bwd: the multipliers of the f32 kernel (rows of A in A B^T, rows of B in A^T B with split-K) and
  colsum_mul_partial_kernel / colsum_reduce_kernel with the multiplier."""
  batch, d = case
  L, lib = _lib()
  c = hb.cross_bwd_case(batch, d, _rng("crossbwd32", case))
  s = L.current_stream()
  for off in (0, 4):
    x0, x, w, b, dy = _dev(c["x0"], off), _dev(c["x"]), _dev(c["w"]), _dev(c["bias"]), _dev(c["dy"], off)
    ws, nb = _ws(lib.tfrs_cross_bwd_workspace_bytes(batch, d, 0))
    for with_db in (True, False):
      dx0, dx, dw, db = _Out(batch * d), _Out(batch * d), _Out(d * d), (_Out(d) if with_db else None)
      ws.fill_(0xFF)
      L.check(lib.tfrs_cross_bwd(_p(x0), _p(x), _p(w), _p(b), c["diag"], _p(dy), batch, d, _p(dx0), _p(dx), _p(dw), _p(db),
                                 _p(ws), nb, s))
      tag = f"cross_bwd {case} off={off}"
      dx0.check(tag + " dx0", c["dx0"])
      dx.check(tag + " dx", c["dx"])
      dw.check(tag + " dkernel", c["dw"])
      if db is not None:
        db.check(tag + " dbias", c["db"])


# ------------------------------------------------------------------------------------------ the f32 kernel, forward
@pytest.mark.parametrize("off", hb.FWD32_OFFSETS)
@pytest.mark.parametrize("family", ["int", "sel_a", "sel_b"])
@pytest.mark.parametrize("case", hb.FWD32, ids=_ids)
def test_forward_products_f32(case, family, off):
  """tfrs_dense_fwd, tfrs_dense_fwd_act (f16 = 0) and tfrs_compute_scores (f16 = 0) at K and M / N around the tile."""
  m, n, k = case
  L, lib = _lib()
  s = L.current_stream()
  c = hb.product(family, m, n, k, _rng("fwd32", family, case))
  bias = hb.small_ints((n,), _rng("bias32", case), -50, 50) if family == "int" else None
  pre = c["ref"] + (hb.f64(bias) if bias is not None else 0.0)
  x, w, wt, b = _dev(c["a"], off), _dev(c["b"], off), _dev(c["b"].T, off), _dev(bias)
  out = _Out(m * n)
  L.check(lib.tfrs_dense_fwd(_p(x), _p(w), _p(b), m, k, n, _p(out), s))
  out.check(f"dense_fwd {family} {case}", pre)
  for code in (0, 1):
    out, pre_out = _Out(m * n), _Out(m * n)
    L.check(lib.tfrs_dense_fwd_act(_p(x), _p(w), _p(b), m, k, n, code, _p(out), _p(pre_out), 0, None, 0, s))
    out.check(f"dense_fwd_act f32 act={code} {family} {case}", hb.relu(pre) if code else pre)
    pre_out.check(f"dense_fwd_act f32 pre {family} {case}", pre)
  out = _Out(m * n)
  L.check(lib.tfrs_compute_scores(_p(x), _p(wt), m, n, k, _p(out), 0, None, 0, s))
  out.check(f"compute_scores f32 {family} {case}", c["ref"])


@pytest.mark.parametrize("off", hb.FWD32_OFFSETS)
@pytest.mark.parametrize("case", hb.CROSS_FWD32, ids=_ids)
def test_cross_fwd_f32(case, off):
  batch, d = case
  L, lib = _lib()
  s = L.current_stream()
  lin = hb.cross_fwd_case(batch, d, _rng("cross32", case))
  act = hb.cross_fwd_case(batch, d, _rng("cross32", case), relu_act=True)
  x0, x, w, b = _dev(lin["x0"]), _dev(lin["x"], off), _dev(lin["w"], off), _dev(lin["bias"])
  y = _Out(batch * d)
  L.check(lib.tfrs_cross_fwd(_p(x0), _p(x), _p(w), _p(b), lin["diag"], batch, d, _p(y), s))
  y.check(f"cross_fwd {case}", lin["y"])
  for code, c in ((1, act), (0, lin)):
    y, pre = _Out(batch * d), _Out(batch * d)
    L.check(lib.tfrs_cross_fwd_act(_p(x0), _p(x), _p(x), d, _p(w), _p(b), c["diag"], code, batch, d, _p(y), _p(pre), 0,
                                   None, 0, s))
    y.check(f"cross_fwd_act f32 act={code} {case}", c["y"])
    pre.check(f"cross_fwd_act f32 pre {case}", c["pre"])


# ------------------------------------------------------------------------------------------ the pointwise backward
@pytest.mark.parametrize("count", hb.MUL_COUNTS + (hb.BIG_COUNT,))
def test_act_pointwise_bwd(count):
  """act_pointwise_bwd_kernel: each of its three optional outputs alone and together, identity and relu, from the
  pre-activation and from the output, with and without x0, from pointers on and off a 16-byte boundary."""
  L, lib = _lib()
  s = L.current_stream()
  rng = _rng("pointwise", count)
  pre, dy, x0, x = (hb.small_ints((count,), rng, -9, 9) for _ in range(4))
  diag = 0.5
  masks = range(1, 8) if count != hb.BIG_COUNT else (7,)
  for off in (0, 4):
    t_pre, t_dy, t_x0, t_x = _dev(pre, off), _dev(dy), _dev(x0, off), _dev(x)
    for act, from_out in ((0, 0), (1, 0), (1, 1), (0, 1)):
      p = hb.relu(hb.f64(pre)) if from_out and act else hb.f64(pre)       # what the `pre` argument holds
      given = _dev(p, off) if from_out and act else t_pre
      grad = (p > 0).astype(np.float64) if act else np.ones(count)
      val = hb.relu(p) if act else p
      for with_x0 in (True, False):
        x0v = hb.f64(x0) if with_x0 else np.ones(count)
        for mask in masks:
          if mask & 4 and not with_x0:
            continue                                                        # (dxd needs x0)
          dp, dx0, dxd = (_Out(count, o) if mask & bit else None for bit, o in ((1, 0), (2, off), (4, 0)))
          L.check(lib.tfrs_act_pointwise_bwd(act, from_out, _p(given), _p(t_dy), _p(t_x0 if with_x0 else None), _p(t_x),
                                             diag, count, _p(dp), _p(dx0), _p(dxd), s))
          tag = f"pointwise count={count} off={off} act={act} from_out={from_out} x0={with_x0} mask={mask}"
          if dp is not None:
            dp.check(tag + " dp", hb.f64(dy) * x0v * grad)
          if dx0 is not None:
            dx0.check(tag + " dx0", hb.f64(dy) * (val + diag * hb.f64(x)))
          if dxd is not None:
            dxd.check(tag + " dxd", hb.f64(dy) * (1.0 + diag * x0v))
