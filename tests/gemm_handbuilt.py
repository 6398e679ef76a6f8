"""Hand-built operands for the GEMM kernels (csrc/gemm16.hip; ``gemm_kernel`` and its helpers in csrc/interaction.hip)
whose products are EXACT in float32 in any summation order, and a Python restatement of the launch planners
(``tfrs_gemm_plan``).  tests/test_gemm_handbuilt_host.py proves every property from the arrays alone and compares the
restated planner with the library's; tests/test_gemm_layout_gpu.py compares the kernels with the float64 products bit
for bit.  Pure numpy at import.

Two families.

integer    Every operand entry (after the fused multiplier) is an integer with |v| <= 1023.  The power-of-two row /
           column scale of ``g16_scale_of`` puts the largest magnitude of a row in [2^9, 2^10): a 10-bit integer times
           a power of two is an fp16 number, so the hi image is exact and the lo image is zero.  Every epilogue operand
           is an integer and ``diag`` is 0.25 or 0.5, so every partial result of an output is a multiple of 0.25; with
           the sum of the ABSOLUTE values of all terms of an output below 2^22 (``EXACT_BOUND``) each of them has at
           most 24 significant bits: exact in float32 whatever the order, fused or not.
selection  One operand is a signed one-hot selection (at most one nonzero, +-1 or +-2, per output column / row), the
           other holds multiples of 2^-12 below 1024 (times a power of two per row): 22 significant bits, so
           ``hi + lo`` reproduces the scaled value exactly and lo is NOT zero.  An output is one product by +-1 / +-2:
           a signed gather of the dense operand, exact, and a wrong entry names its source.
"""

import numpy as np

EXACT_BOUND = float(2 ** 22)
AT, BT, AMUL, BMUL, EPI, BIAS, ACT = 1, 2, 4, 8, 16, 32, 64
KIND_ROWS, KIND_COLS, KIND_KSM1, KIND_KSM2 = 0, 1, 2, 3


def case_rng(*key):
  import zlib
  return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------ the planners, restated
def _ceil(a, b):
  return (a + b - 1) // b


def g16_splits(m, n, k, splitk=None):
  tiles = _ceil(m, 256) * _ceil(n, 256)
  if tiles >= 512 or k < 8192:
    return 1
  if splitk:
    return max(1, int(splitk))
  best, best_eff = 1, 0.0
  for s in range(2, (128 if tiles < 8 else 16) + 1):
    if k // s < 2048:
      break
    waves = tiles * s / 256.0
    eff = waves if waves <= 1.0 else waves / float(int(waves + 0.999999))
    if eff > best_eff + 0.02:
      best_eff, best = eff, s
  return best


def vec_ok(ld, low, mul_low):
  return int(ld % 4 == 0 and low % 16 == 0 and mul_low % 16 == 0)


def row_prep(k, kp, low, mul_low):
  """(steps, v2, waves) of the single-pass K-step-major row prep; steps == 0: the two-pass kernel."""
  nq4 = (kp // 16 + 3) // 4
  steps = (nq4 + 7) // 8
  vec = k >= 4 and vec_ok(k, low, mul_low)
  vec2 = (not vec) and k % 4 == 2 and k >= 6 and low % 8 == 0 and mul_low % 8 == 0
  if vec2 and steps <= 4:
    return 4, 1, 4
  if vec2 and steps <= 16:
    return 8, 1, 8
  for s in (2, 4, 8, 16):
    if vec and steps <= s:
      return s, 0, 4
  return 0, 0, 4


def _lows(flags, align):
  return (align & 15, (align >> 4) & 15, (align >> 8) & 15 if flags & AMUL else 0,
          (align >> 12) & 15 if flags & BMUL else 0)


def plan_f16(m, n, k, flags=0, align=0, tile=0, splitk=None):
  la, lb, lam, lbm = _lows(flags, align)
  mp, np_, kp = _ceil(m, 256) * 256, _ceil(n, 256) * 256, _ceil(k, 64) * 64
  nsplit = g16_splits(m, n, k, splitk)
  split = nsplit > 1 and not flags & (EPI | BIAS | ACT) and tile != 128
  big = (tile == 256 or (tile != 128 and (mp // 256) * (np_ // 256) >= 512) or split) and n < (1 << 23)
  kb = 16 if big else kp
  nk_all = kp // 16
  kt_per = _ceil(nk_all, nsplit) if split else 0
  slices = _ceil(nk_all, kt_per) if split else 1
  out = [int(big), kp, mp, np_, kb, _ceil(k, 256), nsplit, kt_per, slices,
         nk_all - (slices - 1) * kt_per if split else nk_all]
  for cols, ld, low, mlow in ((bool(flags & AT), m if flags & AT else k, la, lam),
                              (not flags & BT, k if flags & BT else n, lb, lbm)):
    o = [1 if cols else 0, 0, 0, 0]
    if not cols and kb == 16:
      steps, v2, waves = row_prep(k, kp, low, mlow)
      o = [KIND_KSM1 if steps else KIND_KSM2, steps, v2, waves]
    out += o + [vec_ok(ld, low, mlow)]
  return out


def splitk_slices_f32(m, n, k):
  tiles = _ceil(m, 128) * _ceil(n, 128)
  if tiles >= 256 or k < 2048:
    return 1
  want = min(_ceil(1024, tiles), k // 1024, max(1, (16 << 20) // max(1, m * n)))
  return max(1, want)


def plan_f32(m, n, k, flags=0, align=0):
  la, lb, lam, lbm = _lows(flags, align)
  slices = splitk_slices_f32(m, n, k) if flags & AT else 1
  kper = used = 0
  if slices > 1:
    kper = _ceil(_ceil(k, slices), 16) * 16
    used = _ceil(k, kper)
  else:
    used = 1
  out = [slices, kper, used, k - (used - 1) * kper if slices > 1 else k,
         vec_ok(m if flags & AT else k, la, lam), vec_ok(k if flags & BT else n, lb, lbm),
         _ceil(m, 128) * _ceil(n, 128)]
  return out + [0] * 13


def plan(f16, m, n, k, flags=0, align=0, tile=0, splitk=None):
  return plan_f16(m, n, k, flags, align, tile, splitk) if f16 else plan_f32(m, n, k, flags, align)


def describe(f16, m, n, k, flags=0, align=0, tile=0, splitk=None):
  """The plan as a dict with names (what the geometry table of the host test speaks about)."""
  p = plan(f16, m, n, k, flags, align, tile, splitk)
  if not f16:
    return dict(zip(("slices", "kper", "used", "last", "a_vec", "b_vec", "tiles"), p))
  d = dict(zip(("big", "kp", "mp", "np", "kb", "nslab", "nsplit", "kt_per", "slices", "last"), p))
  for name, o in (("a", p[10:15]), ("b", p[15:20])):
    d[name] = dict(zip(("kind", "steps", "v2", "waves", "vec"), o))
  d["count"] = m * n
  return d


# ------------------------------------------------------------------------------------------ where things are cut
def k_cuts(k, extra=()):
  """The k indices next to every cut a product of length k can have: both ends, kp, the 16-, 32- and 64-wide K steps
  around them, the 256-row slabs, and the cuts passed in ``extra`` (slice starts)."""
  marks = {0, k, _ceil(k, 64) * 64} | {c for c in extra}
  marks |= {q for q in range(256, k, 256)} if k <= 4096 else {256, 512, (k // 256) * 256}
  out = set()
  for c in marks:
    out |= {c - 17, c - 16, c - 2, c - 1, c, c + 1, c + 15, c + 16}
  return sorted(i for i in out if 0 <= i < k)


def slice_cuts(f16, m, n, k, flags=0, tile=0, splitk=None):
  p = plan(f16, m, n, k, flags, 0, tile, splitk)
  if f16:
    return [s * p[7] * 16 for s in range(1, p[8])] if p[7] else []
  return [s * p[1] for s in range(1, p[2])] if p[1] else []


# ------------------------------------------------------------------------------------------ integer family
PEAKS_A = (1023, 0, 200, 37, 0, 512)
PEAKS_B = (511, 0, 64, 9, 0, 256)


def int_rows(rows, k, rng, cuts=(), peaks=PEAKS_A, zero_row=None, edge=7):
  """[rows, k] integers (float32): a background in [-3, 3]; at the first and last k of every K step of 16 a nonzero
  value of magnitude 5 .. 4 + edge that differs from its neighbours' along both axes; next to every cut of ``cuts``
  a value 16 + (position in the list) on the rows at tile edges; one peak per row from ``peaks`` (0: none), so that
  the rows' maxima -- their power-of-two scales -- differ; one all-zero row."""
  z = rng.integers(-3, 4, (rows, k), dtype=np.int16)
  ii = np.arange(rows, dtype=np.int32)[:, None]
  for first in (0, 15):                       # (only the edge columns are touched: the d x d weights are large)
    kk = np.arange(first, k, 16, dtype=np.int32)[None, :]
    sign = np.where((ii * 7 + kk * 3) % 5 < 2, -1, 1)
    z[:, first::16] = sign * (5 + (3 * ii + 5 * (kk // 16) + kk % 2) % edge)
  cuts = [c for c in cuts if 0 <= c < k]
  edge_rows = [r for r in sorted({0, rows - 1} | {t + d for t in range(0, rows + 1, 128) for d in (-1, 0)}) if 0 <= r < rows]
  for r in edge_rows:
    for idx, c in enumerate(cuts):
      z[r, c] = (16 + (idx + r) % 48) * (1 if (idx + r) % 3 else -1)
  for r in range(rows):
    p = peaks[r % len(peaks)]
    if p:
      z[r, (7 * r + 3) % k] = p if r % 2 else -p
  if zero_row is None:
    zero_row = rows // 2
  if rows > 2:
    z[zero_row] = 0
  return z.astype(np.float32)


def factor(z, rng):
  """z = dy * x0 entry by entry (integers): the fused multiplier of the Cross backward.  x0 is +-2 where z is even
  and nonzero, +-1 elsewhere -- and +-3 against dy = 0 where z is 0."""
  zi = z.astype(np.int64)
  s = np.where(rng.integers(0, 2, z.shape) == 1, 1, -1)
  x0 = np.where((zi % 2 == 0) & (zi != 0), 2 * s, s)
  x0 = np.where(zi == 0, 3 * s, x0)
  dy = zi // x0
  assert np.array_equal(dy * x0, zi)
  return dy.astype(np.float32), x0.astype(np.float32)


def small_ints(shape, rng, lo=-3, hi=3):
  return rng.integers(lo, hi + 1, shape).astype(np.float32)


def abs_terms(a, b):
  """sum_k |a||b| per output, float64 (a [m, k], b [k, n])."""
  return np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))


def f64(a):
  return a.astype(np.float64)


def relu(v):
  return np.maximum(v, 0.0)


# ------------------------------------------------------------------------------------------ selection family
ROW_EXP = (0, -3, 2, 5, -7, 1)


def dense_rows(rows, k, rng, zero_row=None):
  """[rows, k] float32: multiples of 2^-12 below 1024 with the row's largest magnitude in [512, 1024), times a power
  of two per row.  ``scaled_rows`` gives the values in the scaled domain back."""
  sv = rng.integers(-(2 ** 21) + 1, 2 ** 21, (rows, k)).astype(np.float64) * 2.0 ** -12      # |sv| < 512
  for r in range(rows):
    top = (2 ** 21 + int(rng.integers(1, 2 ** 21))) * 2.0 ** -12                              # [512, 1024), 22 bits
    sv[r, (5 * r + 1) % k] = top if r % 2 else -top
  e = np.array([ROW_EXP[r % len(ROW_EXP)] for r in range(rows)], np.float64)
  v = sv * 2.0 ** e[:, None]
  if rows > 2:
    v[rows // 2 if zero_row is None else zero_row] = 0.0
  out = v.astype(np.float32)
  assert np.array_equal(out.astype(np.float64), v)
  return out


def scale_of(maxabs):
  """``g16_scale_of``: the power of two that puts maxabs in [2^9, 2^10) (1 for ~zero), per entry of a float32 array."""
  e = (np.asarray(maxabs, np.float32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
  ok = (e >= 27) & (e < 255)
  s = np.where(ok, (np.uint32(263) - np.where(ok, e, 127)) << np.uint32(23), np.float32(1.0).view(np.uint32))
  return s.astype(np.uint32).view(np.float32)


def split_hi_lo(rows_f32):
  """The hi / lo images of an operand given as [rows, k] (k along the image row), restated with numpy float16."""
  s = scale_of(np.abs(rows_f32).max(axis=1))[:, None]
  sv = (rows_f32 * s).astype(np.float32)
  hi = sv.astype(np.float16)
  lo = (sv - hi.astype(np.float32)).astype(np.float16)
  return sv, hi, lo


def selection(k, cols, rng, sources=()):
  """[k, cols]: column j has one nonzero, +-1 or +-2, at row src[j] (-1: an all-zero column).  ``sources`` come
  first (the planted k positions), the rest is random."""
  sources = [int(c) for c in sources if 0 <= c < k]
  if len(sources) >= cols:     # more planted positions than columns: take them evenly, both ends included
    src = np.array([sources[(i * (len(sources) - 1)) // max(1, cols - 1)] for i in range(cols)], np.int64)
  else:
    src = np.concatenate([np.array(sources, np.int64), rng.integers(0, k, cols - len(sources))])
  val = np.array([(1.0, -1.0, 2.0, -2.0)[j % 4] for j in range(cols)], np.float32)
  if cols > 3:
    src[cols // 3] = -1
  sel = np.zeros((k, cols), np.float32)
  live = src >= 0
  sel[src[live], np.flatnonzero(live)] = val[live]
  return sel, src, np.where(live, val, 0.0).astype(np.float32)


def dense_plain(rows, k, rng):
  """``dense_rows`` without the per-row powers of two and with a value in [512, 1024) in every row AND every column:
  an operand that one product scales by rows and another by columns (dy of the Dense backward)."""
  sv = rng.integers(-(2 ** 21) + 1, 2 ** 21, (rows, k)).astype(np.float64) * 2.0 ** -12
  tops = [(r, (5 * r + 1) % k) for r in range(rows)] + [((5 * c + 1) % rows, c) for c in range(k)]
  for i, (r, c) in enumerate(tops):
    top = (2 ** 21 + int(rng.integers(1, 2 ** 21))) * 2.0 ** -12
    sv[r, c] = top if i % 2 else -top
  out = sv.astype(np.float32)
  assert np.array_equal(out.astype(np.float64), sv)
  return out


# ------------------------------------------------------------------------------------------ products and entry points
def all_cuts(m, n, k, tile=0):
  """Every k the launchers cut a product of length k at, for both GEMMs: see ``k_cuts``."""
  return k_cuts(k, slice_cuts(1, m, n, k, 0, tile) + slice_cuts(0, m, n, k, AT))


def _edge(k):
  return 7 if k <= 40000 else 3


def product(family, m, n, k, rng, tile=0):
  """Logical A [m, k] and B [k, n] of one family ("int", "sel_b": dense A and selection B, "sel_a": the reverse),
  the float64 product and the largest sum of |terms|."""
  cuts = all_cuts(m, n, k, tile)
  if family == "int":
    a = int_rows(m, k, rng, cuts, PEAKS_A, edge=_edge(k))
    b = np.ascontiguousarray(int_rows(n, k, rng, cuts, PEAKS_B, edge=_edge(k)).T)
    return dict(a=a, b=b, ref=f64(a) @ f64(b), terms=float(abs_terms(a, b).max()))
  if family == "sel_b":
    a = dense_rows(m, k, rng)
    b, src, val = selection(k, n, rng, cuts)
    gather = np.where(src >= 0, f64(a)[:, np.maximum(src, 0)] * f64(val), 0.0)
  else:
    bt = dense_rows(n, k, rng)
    st, src, val = selection(k, m, rng, cuts)
    a, b = np.ascontiguousarray(st.T), np.ascontiguousarray(bt.T)
    gather = np.where(src >= 0, f64(bt)[:, np.maximum(src, 0)] * f64(val), 0.0).T
  ref = f64(a) @ f64(b)
  assert np.array_equal(ref, gather)            # a signed gather of the dense operand
  return dict(a=a, b=b, ref=ref, src=src, val=val, terms=0.0)


PEAKS_X = (255, 0, 100, 37, 0, 128)
DIAGS = (0.5, 0.25)


def cross_fwd_case(batch, d, rng, tile=0, relu_act=False):
  """Cross.call on integers: u = x W + b + diag x (or relu(x W + b) + diag x), y = x0 u + x."""
  cuts = all_cuts(batch, d, d, tile)
  x = int_rows(batch, d, rng, cuts, PEAKS_A)
  w = np.ascontiguousarray(int_rows(d, d, rng, cuts, PEAKS_B).T)
  x0, bias, diag = small_ints((batch, d), rng), small_ints((d,), rng, -50, 50), DIAGS[(batch + d) % 2]
  pre = f64(x) @ f64(w) + f64(bias)
  u = (relu(pre) if relu_act else pre) + diag * f64(x)
  y = f64(x0) * u + f64(x)
  terms = np.abs(f64(x0)) * (abs_terms(x, w) + np.abs(f64(bias)) + diag * np.abs(f64(x))) + np.abs(f64(x))
  return dict(x0=x0, x=x, w=w, bias=bias, diag=diag, pre=pre, u=u, y=y, terms=float(terms.max()))


def factor_small(z, rng):
  """z = dy * x0 with |dy| <= 3 (the multiplier x0 carries the magnitude): dy divides z; where z is 0 either factor
  is 0, by turns."""
  zi = z.astype(np.int64)
  s = np.where(rng.integers(0, 2, z.shape) == 1, 1, -1)
  dy = np.where(zi % 3 == 0, 3 * s, np.where(zi % 2 == 0, 2 * s, s))
  x0 = zi // dy
  zero = zi == 0
  turn = (np.arange(z.size).reshape(z.shape) % 2 == 0)
  dy = np.where(zero & turn, 0, dy)
  x0 = np.where(zero & turn, 5 * s, x0)
  assert np.array_equal(dy * x0, zi) and np.abs(dy).max() <= 3
  return dy.astype(np.float32), x0.astype(np.float32)


def _k_major(rows_k, cols, rng, cuts, peaks, edge):
  return np.ascontiguousarray(int_rows(cols, rows_k, rng, cuts, peaks, edge=edge).T)


def cross_bwd_case(batch, d, rng, tile=0):
  """The Cross backward on integers; dz = dy * x0 is what the fused multiplier builds.  The cuts are planted along
  the longer of the two K axes (d for dx, batch for dW)."""
  if batch > d:
    cuts = all_cuts(d, d, batch, tile)
    dz = _k_major(batch, d, rng, cuts, PEAKS_A, _edge(batch))
    x = _k_major(batch, d, rng, cuts, PEAKS_X, _edge(batch))
  else:
    cuts = all_cuts(batch, d, d, tile)
    dz = int_rows(batch, d, rng, cuts, PEAKS_A)
    x = int_rows(batch, d, rng, cuts, PEAKS_X)
  w = int_rows(d, d, rng, all_cuts(batch, d, d, tile), PEAKS_B)       # rows of W: the image rows of the dx product
  dy, x0 = factor_small(dz, rng)
  bias, diag = small_ints((d,), rng, -50, 50), DIAGS[(batch + d) % 2]
  wf = f64(w)                                   # (converted once: the weights of the largest cases are 8196 x 8196)
  u = f64(x) @ wf + f64(bias) + diag * f64(x)
  dx0 = f64(dy) * u
  dx = f64(dz) @ wf.T + f64(dy) + diag * f64(dz)
  dw = f64(x).T @ f64(dz)
  db = f64(dz).sum(axis=0)
  add = small_ints((batch, d), rng, -9, 9)
  np.abs(wf, out=wf)
  ax, adz = np.abs(f64(x)), np.abs(f64(dz))
  terms = max(float((np.abs(f64(dy)) * (ax @ wf + np.abs(f64(bias)) + diag * ax)).max()) + 9 + float(np.abs(dx).max()),
              float((adz @ wf.T + np.abs(f64(dy)) + diag * adz).max()),
              float((ax.T @ adz).max()), float(adz.sum(axis=0).max()))
  return dict(x0=x0, x=x, w=w, bias=bias, diag=diag, dy=dy, dz=dz, u=u, dx0=dx0, dx=dx, dw=dw, db=db, add=add,
              terms=terms)


def dense_bwd_case(family, batch, din, dout, rng, tile=0):
  """dx = dy W^T (+ addend), dW = x^T dy, db = column sums of dy.  "sel": W and x are selections, dy is dense."""
  if family == "int":
    if batch > max(din, dout):
      cuts = all_cuts(din, dout, batch, tile)
      dy = _k_major(batch, dout, rng, cuts, PEAKS_B, _edge(batch))
      x = _k_major(batch, din, rng, cuts, PEAKS_A, _edge(batch))
    else:
      cuts = all_cuts(batch, din, dout, tile)
      dy, x = int_rows(batch, dout, rng, cuts, PEAKS_A), int_rows(batch, din, rng, (), PEAKS_X)
    w = int_rows(din, dout, rng, all_cuts(batch, din, dout, tile), PEAKS_B)
    add = small_ints((batch, din), rng, -9, 9)
    terms = max(float(abs_terms(dy, w.T).max()) + 9, float(abs_terms(x.T, dy).max()),
                float(np.abs(f64(dy)).sum(axis=0).max()))
  else:
    dy = dense_plain(batch, dout, rng)
    w = np.ascontiguousarray(selection(dout, din, rng, all_cuts(batch, din, dout, tile))[0].T)
    x = np.ascontiguousarray(selection(batch, din, rng, all_cuts(din, dout, batch, tile))[0])
    add, terms = None, 0.0
  dx = f64(dy) @ f64(w).T
  return dict(x=x, w=w, dy=dy, add=add, dx=dx, dx_add=None if add is None else dx + f64(add), dw=f64(x).T @ f64(dy),
              db=f64(dy).sum(axis=0) if family == "int" else None, terms=terms)


def exact_f32(ref):
  """Every entry of a float64 reference is a float32 number."""
  with np.errstate(over="ignore"):
    return bool(np.array_equal(ref.astype(np.float32).astype(np.float64), ref))


# ------------------------------------------------------------------------------------------ shapes
# (m, n) pairs dealt over the K list of the row-prep table: every m, n of {1, 127, 128, 129, 255, 256, 257, 300}
ROWPREP_K = {64: (1, 300), 300: (127, 129), 2048: (128, 255), 4096: (129, 1), 4100: (255, 128), 8192: (256, 257),
             1030: (257, 127), 2050: (300, 256), 5082: (129, 131), 8196: (127, 3), 8194: (3, 129), 13: (300, 300),
             1: (257, 257)}
# (k, byte offset of the operand, what the plan says): pointers 4 / 8 / 12 bytes into the storage
ROWPREP_OFFSETS = [(300, 4, "fallback"), (300, 8, "fallback"), (1030, 8, "v2"), (1030, 4, "fallback"), (1030, 12, "fallback"),
                   (2048, 12, "fallback")]
# what the Cross backward (the fused multiplier: d x d weights, k = d) runs at each k: batch sizes stay small
ROWPREP_MUL_BATCH = {64: 300, 300: 129, 2048: 5, 4096: 3, 4100: 2, 8192: 1, 1030: 127, 2050: 3, 5082: 2, 8196: 1,
                     8194: 1, 13: 257, 1: 128}
SPLIT16 = [(129, 131, 12289), (129, 131, 12288), (257, 129, 8192), (130, 3, 20000), (300, 257, 16385), (129, 131, 8191), (129, 131, 8192)]
SMALL16 = [(127, 129, 31), (128, 127, 32), (129, 128, 33), (127, 128, 63), (128, 129, 64), (129, 127, 65),
           (257, 300, 33), (1, 1, 1)]
SPLIT32 = [(129, 131, 2047), (129, 131, 2048), (129, 131, 2049), (129, 131, 3073), (5, 3, 2100), (13, 512, 4097),
           (130, 126, 3072)]
FWD32 = [(127, 129, 15), (128, 127, 16), (129, 128, 17), (127, 128, 33), (129, 130, 16), (300, 257, 34), (1, 1, 1)]
MUL_COUNTS = (1, 3, 4, 5, 1023, 1024, 1027)
BIG_COUNT = 256 * 32 * 256 * 4 + 5        # the grid-stride loops of both element-wise kernels take a second round


# ------------------------------------------------------------------------------------------ what the GPU file launches
# Every list below parametrises one test of tests/test_gemm_layout_gpu.py; ``products`` turns them into the GEMM
# products (f16, m, n, k, flags, align, tile) those tests launch, which is what the geometry table of the host test
# is asked about.
SCORES16 = ([(m, n, k, 256, 0, 0) for k, (m, n) in ROWPREP_K.items()] +
            [(129, 131, k, 256, off, 0) for k, off, _ in ROWPREP_OFFSETS] +
            [(131, 129, k, 256, 0, off) for k, off, _ in ROWPREP_OFFSETS[:4]] +
            [(m, n, k, 128, 0, 0) for m, n, k in SMALL16] + [(129, 131, 300, 128, 4, 8)] +
            [(m, n, k, 0, 0, 0) for m, n, k in SPLIT16])
# (batch = m, dout = n, din = k, tile, bias, act, byte offset of the kernel)
DENSE_FWD16 = ([(m, n, k, 0, 0, 0, 0) for m, n, k in SPLIT16] +
               [(129, 131, 300, 256, 1, 0, 0), (129, 132, 300, 256, 1, 1, 0), (129, 132, 300, 256, 0, 0, 4),
                (257, 300, 33, 128, 1, 1, 0), (127, 128, 64, 128, 1, 0, 0), (128, 64, 257, 128, 0, 1, 8),
                (300, 257, 513, 256, 1, 1, 0), (1, 1, 1, 128, 1, 1, 0)])
# (batch, d, tile)
CROSS_FWD16 = [(129, 127, 128), (127, 129, 256), (300, 257, 256), (257, 300, 128), (1, 1, 256), (128, 64, 128)]
# (batch, d, tile): the fused multiplier at every k = d of the row-prep table, and the small kernel's layouts
CROSS_BWD16 = ([(b, d, 256) for d, b in ROWPREP_MUL_BATCH.items()] +
               [(129, 127, 128), (257, 129, 128), (300, 33, 128), (12289, 129, 0), (8192, 132, 0)])
# (batch, din, dout, tile)
DENSE_BWD16 = [(12289, 129, 131, 0), (8192, 257, 129, 0), (20000, 130, 3, 0), (300, 129, 131, 128), (257, 300, 33, 256),
               (513, 128, 132, 256), (1, 1, 1, 128)]
# f32 kernel: (batch, din, dout) of the backward = the dW-shaped product (din, dout, batch)
DENSE_BWD32 = [(k, m, n) for m, n, k in SPLIT32] + [(300, 129, 131), (17, 128, 127), (1, 1, 1)]
CROSS_BWD32 = [(2047, 129), (2048, 129), (2049, 130), (3073, 131), (300, 128), (33, 127), (1, 1)]
CROSS_FWD32 = [(127, 15), (128, 16), (129, 17), (127, 33), (129, 128), (300, 129), (1, 1)]
BIG_MUL = (129057, 65)                    # batch * d > 256 * 32 * 256 * 4, and not a multiple of 4
BWD32_OFFSETS = (0, 4, 8)
FWD32_OFFSETS = (0, 4)


def products():
  out = []
  for m, n, k, tile, offa, offb in SCORES16:
    out.append((1, m, n, k, BT, offa | offb << 4, tile))
  for m, n, k, tile, bias, act, offb in DENSE_FWD16:
    out.append((1, m, n, k, (BIAS if bias else 0) | (ACT if act else 0), offb << 4, tile))
  for b, d, tile in CROSS_FWD16:
    out += [(1, b, d, d, EPI | BIAS, 0, tile), (1, b, d, d, EPI | BIAS | ACT, 0, tile)]
  for b, d, tile in CROSS_BWD16:
    out += [(1, b, d, d, EPI | BIAS, 0, tile), (1, b, d, d, BT | AMUL | EPI, 0, tile), (1, d, d, b, AT | BMUL, 0, tile)]
  for b, din, dout, tile in DENSE_BWD16:
    out += [(1, b, din, dout, BT, 0, tile), (1, b, din, dout, BT | EPI, 0, tile), (1, din, dout, b, AT, 0, tile)]
  for b, din, dout in DENSE_BWD32:
    for off in BWD32_OFFSETS:
      out += [(0, b, din, dout, BT, off << 4, 0), (0, din, dout, b, AT, off | off << 4, 0)]
  for b, d in CROSS_BWD32:
    out += [(0, b, d, d, EPI | BIAS, 0, 0), (0, b, d, d, BT | AMUL | EPI, 0, 0), (0, d, d, b, AT | BMUL, 0, 0)]
  for m, n, k in FWD32:
    for off in FWD32_OFFSETS:
      out += [(0, m, n, k, BIAS | ACT, off | off << 4, 0), (0, m, n, k, BT, off | off << 4, 0)]
  for b, d in CROSS_FWD32:
    for off in FWD32_OFFSETS:
      out.append((0, b, d, d, EPI | BIAS | ACT, off | off << 4, 0))
  for b, d in [(c, 1) for c in MUL_COUNTS] + [BIG_MUL]:
    out += [(1, b, d, d, EPI | BIAS, 0, 0), (1, b, d, d, BT | AMUL | EPI, 0, 0), (1, d, d, b, AT | BMUL, 0, 0)]
  return out
