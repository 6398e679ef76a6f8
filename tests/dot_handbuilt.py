"""Hand-built inputs for the DotInteraction kernels (csrc/interaction.hip), numpy only.

Every input is ``x[b, i, k] = m * 2^(e_b + g_i)`` with an integer ``|m| <= 7``, a per-sample exponent ``e_b`` in
[-20, 20] and a per-feature exponent ``g_i`` in [0, 4]; every gradient entry is ``m' * 2^(e'_b)`` with ``|m'| <= 7``.
Within one sample (and so within one 32-row block of it) every operand is an integer of at most 7 bits times the
sample's power of two, so the split-fp16 kernels hold it exactly in the ``hi`` half (``lo`` = 0) under a per-sample or a
per-block power-of-two scale, and every partial sum of every dot product is an integer below 2^24 times a common power
of two: the f32 MFMA chains and the f32 fma chains are exact in any order, the power-of-two unscale is exact.  Every
kernel route must therefore return the float64 result as VALUES (``array_equal``: the sign of a zero is not pinned).
tests/test_dot_handbuilt_host.py proves these properties from the arrays and proves that the case lists below reach
every (kernel, template arguments) the library's own decision function can choose; tests/test_dot_layout_gpu.py runs
the cases through the C entry points."""

import contextlib
import ctypes
import zlib

import numpy as np

from oracle import feature_interaction as o_fi

# TFRS_DOT_KERNEL_* of include/tfrs_hip.h
REFUSED, NONE, GATHER, MFMA_STAGED, MFMA_DIRECT, F16X3, F16X3_DIRECT, FWD_PC, BWD_MFMA, BWD_DENSE, BWD_PC, BWD_H16 = range(12)
PERSISTENT = (MFMA_STAGED, MFMA_DIRECT, F16X3, F16X3_DIRECT, FWD_PC, BWD_MFMA, BWD_DENSE, BWD_PC, BWD_H16)   # grid-stride over the samples
FOUR_SAMPLES = (MFMA_DIRECT, F16X3_DIRECT)      # ... with a sample per wave of a four-wave workgroup; the others: one per workgroup
EXACT_BOUND = 1 << 24
MAX_M, E_RANGE, G_RANGE = 7, 20, 4
SWITCHES = ("TFRS_DOT_STAGE", "TFRS_DOT_FWD", "TFRS_DOT_BWD")
# every value of the three switches the decision function tells apart (None: unset)
STAGE_VALUES = (None, "0")
FWD_VALUES = (None, "direct", "staged", "f32")
BWD_VALUES = (None, "pc", "dense", "gather")


def case_rng(*key):
  return np.random.default_rng(zlib.crc32(repr(key).encode()))


def padded(d):
  return next(p for p in (8, 16, 32, 64, 128) if d <= p) if d <= 128 else 0


def pairs(f, self_i):
  return f * (f + 1) // 2 if self_i else f * (f - 1) // 2


def out_dim(f, self_i, skip):
  return f * f if skip else pairs(f, self_i)


# ------------------------------------------------------------------------------------------ the packed order
def packed_offset(i, self_i):
  """Where row i of the lower triangle starts in the packed row (row-major; the diagonal only with self interaction)."""
  return i * (i + 1) // 2 if self_i else i * (i - 1) // 2


def packed_index(f, self_i):
  """(rows, cols) of the pairs in packed order: p = packed_offset(i) + j for j <= i (self) or j < i."""
  rows, cols = [], []
  for i in range(f):
    for j in range(i + 1 if self_i else i):
      assert packed_offset(i, self_i) + j == len(rows)
      rows.append(i)
      cols.append(j)
  return np.asarray(rows, np.int64), np.asarray(cols, np.int64)


def keep_mask(f, self_i):
  return np.tril(np.ones((f, f), bool), 0 if self_i else -1)


# ------------------------------------------------------------------------------------------ the operation, float64
def gram(x):
  """x[b] x[b]^T in float64."""
  x = np.asarray(x, np.float64)
  return x @ np.transpose(x, (0, 2, 1))


def forward64(x, self_i, skip):
  """out[b] = the lower triangle of x[b] x[b]^T: packed, or (skip_gather) the f x f matrix with the rest zeroed."""
  x = np.asarray(x, np.float64)
  g = gram(x)
  f = x.shape[1]
  if skip:
    return np.where(keep_mask(f, self_i)[None], g, 0.0).reshape(x.shape[0], f * f)
  r, c = packed_index(f, self_i)
  return g[:, r, c].reshape(x.shape[0], len(r))


def backward64(x, dy, self_i, skip, double_diagonal=True):
  """dx[b] = (L + L^T) x[b] with L the lower triangle holding dy[b] (so a diagonal entry counts twice)."""
  x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
  b, f, _ = x.shape
  low = np.zeros((b, f, f))
  if skip:
    low = np.where(keep_mask(f, self_i)[None], dy.reshape(b, f, f), 0.0)
  else:
    r, c = packed_index(f, self_i)
    low[:, r, c] = dy
  s = low + np.transpose(low, (0, 2, 1))
  if not double_diagonal:
    idx = np.arange(f)
    s[:, idx, idx] = low[:, idx, idx]
  return s @ x


def oracle_forward(x, self_i, skip):
  return o_fi.dot_interaction([x[:, j, :] for j in range(x.shape[1])], self_i, skip)


def oracle_backward(x, dy, self_i, skip):
  return o_fi.dot_interaction_grad([x[:, j, :] for j in range(x.shape[1])], dy, self_i, skip)


def term_sums(x, dy, self_i, skip):
  """Sum of |terms| of every forward and backward entry (float64)."""
  return forward64(np.abs(x), self_i, skip), backward64(np.abs(x), np.abs(dy), self_i, skip)


# ------------------------------------------------------------------------------------------ the inputs
def planted(batch, f):
  """Samples (zero input, zero gradient, zero feature row, zero 32-row block), the zero row and the zero block."""
  assert batch >= 5
  return {"zero_x": 1, "zero_dy": 3, "zero_row": (2, f // 2), "zero_block": (4, ((f + 31) // 32) // 2)}


def build(batch, f, d, self_i, skip, rng):
  """x[batch, f, d] and dy[batch, out_dim] (float32) with their exponents and the float64 results."""
  eb = rng.integers(-E_RANGE, E_RANGE + 1, size=batch)
  gi = rng.integers(0, G_RANGE + 1, size=f)
  edy = rng.integers(-E_RANGE, E_RANGE + 1, size=batch)
  eb[0], eb[batch - 1], gi[0], gi[f - 1] = E_RANGE, -E_RANGE, G_RANGE, 0         # the extremes are present
  if f > 1:
    gi[f - 1], gi[max(0, f - 2)] = 0, G_RANGE
  m = rng.integers(-MAX_M, MAX_M + 1, size=(batch, f, d))
  m[:, :, 0] = np.where(m[:, :, 0] == 0, MAX_M, m[:, :, 0])                       # no feature row is zero by chance
  if d > 1:
    m[:, :, d - 1] = np.where(m[:, :, d - 1] == 0, -MAX_M, m[:, :, d - 1])        # (the last column is never zero)
  n = out_dim(f, self_i, skip)
  mdy = rng.integers(-MAX_M, MAX_M + 1, size=(batch, n))
  mdy = np.where(mdy == 0, 1, mdy) if n else mdy
  p = planted(batch, f)
  m[p["zero_x"]] = 0
  mdy[p["zero_dy"]] = 0
  m[p["zero_row"][0], p["zero_row"][1]] = 0
  nb = (f + 31) // 32
  if nb > 1:
    m[p["zero_block"][0], 32 * p["zero_block"][1]: 32 * p["zero_block"][1] + 32] = 0
  x = (m * np.exp2(eb[:, None, None] + gi[None, :, None])).astype(np.float32)
  dy = (mdy * np.exp2(edy[:, None])).astype(np.float32)
  return {"x": x, "dy": dy, "m": m, "mdy": mdy, "eb": eb, "gi": gi, "edy": edy,
          "out": forward64(x, self_i, skip), "dx": backward64(x, dy, self_i, skip)}


def rounding_inputs(batch, f, d, self_i, skip, rng):
  """N(0, 1) inputs times a per-sample exp(4 N(0, 1)) scale (the rounding cases: gated, not exact)."""
  x = rng.normal(size=(batch, f, d)) * np.exp(4.0 * rng.normal(size=(batch, 1, 1)))
  dy = rng.normal(size=(batch, out_dim(f, self_i, skip))) * np.exp(4.0 * rng.normal(size=(batch, 1)))
  x[1] = 0.0
  dy[3] = 0.0
  return x.astype(np.float32), dy.astype(np.float32)


# ------------------------------------------------------------------------------------------ the library's plan
@contextlib.contextmanager
def switches(stage=None, fwd=None, bwd=None):
  """TFRS_DOT_STAGE / TFRS_DOT_FWD / TFRS_DOT_BWD set for the block and restored after it."""
  from recommenders_amd import _lib
  old = [_lib.get_option(name) for name in SWITCHES]
  try:
    for name, value in zip(SWITCHES, (stage, fwd, bwd)):
      _lib.set_option(name, value)
    yield
  finally:
    for name, value in zip(SWITCHES, old):
      _lib.set_option(name, value)


FIELDS = ("kernel", "dp", "nb", "stage", "blocks", "nfb", "maxe", "nstep", "ney", "nset", "grid", "threads", "lds",
          "lds_limit", "kh", "aux")


def plan_many(shapes):
  """int64[n, 32] for rows of (batch, f, d, self_interaction, skip_gather, strided), under the switches in force."""
  from recommenders_amd import _lib
  a = np.ascontiguousarray(shapes, np.int64).reshape(-1, 6)
  out = np.zeros((len(a), 32), np.int64)
  _lib.check(_lib.load().tfrs_dot_interaction_plan_many(len(a), a.ctypes.data_as(ctypes.c_void_p),
                                                        out.ctypes.data_as(ctypes.c_void_p)))
  return out


def plan(batch, f, d, self_i=False, skip=False, strided=False):
  """{"fwd": {...}, "bwd": {...}} from tfrs_dot_interaction_plan."""
  from recommenders_amd import _lib
  out = (ctypes.c_int64 * 32)()
  _lib.check(_lib.load().tfrs_dot_interaction_plan(batch, f, d, int(self_i), int(skip), int(strided), out))
  v = [int(t) for t in out]
  return {"fwd": dict(zip(FIELDS, v[:16])), "bwd": dict(zip(FIELDS, v[16:]))}


def route_name(direction, r):
  """The (kernel, template arguments) of one half of a plan row, as the case lists spell it."""
  r = dict(zip(FIELDS, (int(t) for t in r))) if not isinstance(r, dict) else r
  k = r["kernel"]
  body = {REFUSED: "refused", NONE: "none", GATHER: "gather",
          MFMA_STAGED: "mfma<%d,%d,staged>" % (r["dp"], r["nb"]), MFMA_DIRECT: "mfma<%d,%d,direct>" % (r["dp"], r["nb"]),
          F16X3: "f16x3<%d,%d>" % (r["dp"], r["nb"]), F16X3_DIRECT: "f16x3_direct<%d,%d,%d>" % (r["dp"], r["nb"], r["blocks"]),
          FWD_PC: "pc<%d,%d>" % (r["nb"], r["nset"]), BWD_MFMA: "mfma<%d,%d>" % (r["dp"], r["nb"]),
          BWD_DENSE: "dense<%d,%d>" % (r["nfb"], r["maxe"]), BWD_PC: "pc<%d>" % r["maxe"],
          BWD_H16: "h16<%d,%d,%d>" % (r["nstep"], r["ney"], r["nset"])}[k]
  assert (direction == "fwd") == (k in (MFMA_STAGED, MFMA_DIRECT, F16X3, F16X3_DIRECT, FWD_PC)) or k <= GATHER
  return direction + "." + body


def variant_name(direction, r):
  """route_name plus what the decision varies without a template argument: the samples per workgroup of the fallback
  backward (4, 2 or 1) and the one-workgroup-per-CU LDS request of the producer / consumer forward."""
  r = dict(zip(FIELDS, (int(t) for t in r))) if not isinstance(r, dict) else r
  name = route_name(direction, r)
  if direction == "bwd" and r["kernel"] == GATHER:
    name += "/%d" % r["aux"]
  if r["kernel"] == FWD_PC and r["lds_limit"] > 80 * 1024:
    name += "/160K"
  return name


def samples_per_trip(r):
  """How many samples one trip of a persistent kernel's grid-stride loop covers."""
  return r["grid"] * (4 if r["kernel"] in FOUR_SAMPLES else 1)


# ------------------------------------------------------------------------------------------ the cases
class Case:
  """One call pair.  ``route``: the (kernel, template arguments) the case is named for, in the direction it says."""

  def __init__(self, route, batch, f, d, self_i=0, skip=0, stage=None, fwd=None, bwd=None, strided=0):
    self.route, self.batch, self.f, self.d = route, batch, f, d
    self.self_i, self.skip, self.strided = int(self_i), int(skip), int(strided)
    self.sw = (stage, fwd, bwd)

  @property
  def direction(self):
    return self.route.split(".")[0]

  @property
  def n(self):
    return out_dim(self.f, self.self_i, self.skip)

  def shape_row(self):
    return (self.batch, self.f, self.d, self.self_i, self.skip, self.strided)

  def planned(self):
    with switches(*self.sw):
      return plan(self.batch, self.f, self.d, self.self_i, self.skip, self.strided)

  def build(self):
    return build(self.batch, self.f, self.d, self.self_i, self.skip, case_rng("dot", self.id))

  @property
  def id(self):
    sw = "".join("," + n[9:].lower() + "=" + v for n, v in zip(SWITCHES, self.sw) if v)
    return "%s:B%d,F%d,D%d,self%d%s%s%s" % (self.route, self.batch, self.f, self.d, self.self_i,
                                            ",skip" if self.skip else "", ",strided" if self.strided else "", sw)

  def __repr__(self):
    return self.id


C = Case
SMALL, LARGE = 67, 579      # LARGE: the routes that need batch >= 512

# One case per (kernel, template arguments) the decision function can choose, forward.  F sits just inside its row
# block (31 / 32 / 33, 64 / 65, 96 / 97, 128), d is the padded width DP or a d < DP that is not a multiple of 4.
FWD_ROUTES = [
    C("fwd.none", SMALL, 1, 8),
    C("fwd.gather", SMALL, 130, 16), C("fwd.gather", SMALL, 5, 129, 1), C("fwd.gather", SMALL, 130, 13, 1, 1),
    # exact-f32 chain, staged copy-out: the default where the split-fp16 operands would spill ...
    C("fwd.mfma<8,1,staged>", SMALL, 31, 3, 1), C("fwd.mfma<8,1,staged>", SMALL, 32, 8),
    C("fwd.mfma<8,2,staged>", SMALL, 33, 8, 1), C("fwd.mfma<8,2,staged>", SMALL, 64, 5),
    C("fwd.mfma<8,3,staged>", SMALL, 65, 7), C("fwd.mfma<8,3,staged>", SMALL, 96, 8, 1),
    C("fwd.mfma<8,4,staged>", SMALL, 97, 8, 1), C("fwd.mfma<8,4,staged>", SMALL, 128, 3),
    C("fwd.mfma<64,4,staged>", SMALL, 97, 64), C("fwd.mfma<64,4,staged>", SMALL, 128, 33, 1),
    C("fwd.mfma<128,2,staged>", SMALL, 33, 128, 1), C("fwd.mfma<128,2,staged>", SMALL, 64, 65),
    # ... and behind TFRS_DOT_FWD=f32 elsewhere
    C("fwd.mfma<16,1,staged>", SMALL, 32, 13, 1, fwd="f32"), C("fwd.mfma<16,2,staged>", SMALL, 33, 16, fwd="f32"),
    C("fwd.mfma<16,3,staged>", SMALL, 96, 12, fwd="f32"), C("fwd.mfma<16,4,staged>", SMALL, 97, 16, 1, fwd="f32"),
    C("fwd.mfma<32,1,staged>", SMALL, 31, 32, fwd="f32"), C("fwd.mfma<32,2,staged>", SMALL, 64, 21, 1, fwd="f32"),
    C("fwd.mfma<32,3,staged>", SMALL, 65, 32, 1, fwd="f32"), C("fwd.mfma<32,4,staged>", SMALL, 128, 20, fwd="f32"),
    C("fwd.mfma<64,1,staged>", SMALL, 32, 64, 1, fwd="f32"), C("fwd.mfma<64,2,staged>", SMALL, 33, 48, fwd="f32"),
    C("fwd.mfma<64,3,staged>", SMALL, 96, 33, fwd="f32"), C("fwd.mfma<128,1,staged>", SMALL, 31, 100, 1, fwd="f32"),
    # direct stores of the f32 chain: skip_gather and TFRS_DOT_STAGE=0
    C("fwd.mfma<8,1,direct>", SMALL, 32, 3, 0, 1), C("fwd.mfma<8,2,direct>", SMALL, 33, 8, 1, 1),
    C("fwd.mfma<8,3,direct>", SMALL, 65, 8, stage="0"), C("fwd.mfma<8,4,direct>", SMALL, 128, 7, 1, stage="0"),
    C("fwd.mfma<16,1,direct>", SMALL, 31, 16, 1, stage="0"), C("fwd.mfma<16,2,direct>", SMALL, 64, 13, 0, 1),
    C("fwd.mfma<16,3,direct>", SMALL, 96, 16, 1, 1), C("fwd.mfma<16,4,direct>", SMALL, 97, 12, stage="0"),
    C("fwd.mfma<32,1,direct>", SMALL, 32, 21, 1, 1), C("fwd.mfma<32,2,direct>", SMALL, 33, 32, stage="0"),
    C("fwd.mfma<32,3,direct>", SMALL, 65, 20, 1, stage="0"), C("fwd.mfma<32,4,direct>", SMALL, 128, 32, 0, 1),
    C("fwd.mfma<64,1,direct>", SMALL, 31, 33, stage="0"), C("fwd.mfma<64,2,direct>", SMALL, 64, 64, 1, 1),
    C("fwd.mfma<64,3,direct>", SMALL, 96, 48, 0, 1), C("fwd.mfma<64,4,direct>", SMALL, 97, 64, 1, stage="0"),
    C("fwd.mfma<128,1,direct>", SMALL, 32, 128, 1, stage="0"), C("fwd.mfma<128,2,direct>", SMALL, 33, 65, 0, 1),
    # split-fp16, staged copy-out: TFRS_DOT_FWD=staged
    C("fwd.f16x3<16,1>", SMALL, 31, 13, fwd="staged"), C("fwd.f16x3<16,2>", SMALL, 64, 16, 1, fwd="staged"),
    C("fwd.f16x3<16,3>", SMALL, 65, 12, 1, fwd="staged"), C("fwd.f16x3<16,4>", SMALL, 128, 16, fwd="staged"),
    C("fwd.f16x3<32,1>", SMALL, 32, 32, 1, fwd="staged"), C("fwd.f16x3<32,2>", SMALL, 33, 21, fwd="staged"),
    C("fwd.f16x3<32,3>", SMALL, 96, 32, fwd="staged"), C("fwd.f16x3<32,4>", SMALL, 97, 20, 1, fwd="staged"),
    C("fwd.f16x3<64,1>", SMALL, 31, 64, 1, fwd="staged"), C("fwd.f16x3<64,2>", SMALL, 64, 33, fwd="staged"),
    C("fwd.f16x3<64,3>", SMALL, 65, 48, 1, fwd="staged"), C("fwd.f16x3<128,1>", SMALL, 32, 65, fwd="staged"),
    C("fwd.f16x3<128,1>", SMALL, 31, 128, 1, fwd="staged"),
    # split-fp16, direct stores: the default off d = 32 and below batch 512
    C("fwd.f16x3_direct<16,1,3>", SMALL, 32, 16), C("fwd.f16x3_direct<16,1,3>", SMALL, 31, 13, 1),
    C("fwd.f16x3_direct<16,2,3>", SMALL, 33, 12, 1), C("fwd.f16x3_direct<16,3,3>", SMALL, 96, 16),
    C("fwd.f16x3_direct<16,4,3>", SMALL, 97, 13), C("fwd.f16x3_direct<16,4,3>", SMALL, 128, 16, 1),
    C("fwd.f16x3_direct<32,1,3>", SMALL, 31, 32), C("fwd.f16x3_direct<32,2,3>", SMALL, 64, 32, 1),
    C("fwd.f16x3_direct<32,2,3>", SMALL, 33, 21), C("fwd.f16x3_direct<32,3,3>", SMALL, 65, 20, 1),
    C("fwd.f16x3_direct<32,4,3>", SMALL, 128, 32, 1), C("fwd.f16x3_direct<32,4,3>", SMALL, 97, 17),
    C("fwd.f16x3_direct<64,1,3>", SMALL, 32, 33, 1), C("fwd.f16x3_direct<64,2,3>", SMALL, 33, 64),
    C("fwd.f16x3_direct<64,2,3>", SMALL, 64, 48, 1), C("fwd.f16x3_direct<64,3,3>", SMALL, 96, 64, 1),
    C("fwd.f16x3_direct<64,3,3>", SMALL, 65, 33), C("fwd.f16x3_direct<128,1,3>", SMALL, 31, 65),
    C("fwd.f16x3_direct<128,1,3>", SMALL, 32, 128, 1), C("fwd.f16x3_direct<128,1,3>", SMALL, 32, 100),
    # producer / consumer: d = 32, two row blocks and more, batch >= 512
    C("fwd.pc<2,4>", LARGE, 33, 32, 1), C("fwd.pc<2,4>", LARGE, 64, 32),
    C("fwd.pc<3,4>", LARGE, 65, 32), C("fwd.pc<3,4>", LARGE, 96, 32, 1),
    C("fwd.pc<4,4>", LARGE, 97, 32, 1), C("fwd.pc<4,4>", LARGE, 108, 32), C("fwd.pc<4,4>", LARGE, 109, 32),     # (80 KiB of LDS and just past it)
    C("fwd.pc<4,4>", LARGE, 128, 32), C("fwd.pc<4,4>", LARGE, 128, 32, 1),
]

# ... and backward.  MAXE edges of the unpack (3072 and 5120 pairs): F = 77 / 78 / 79 and 100 / 101 / 102 with the
# variant that crosses; F = 122 / 123: the edge of the dense tile; F = 128 with self interaction (8256 pairs: past the dense tile, so the gathered kernel).
BWD_ROUTES = [
    C("bwd.none", SMALL, 1, 8),
    C("bwd.gather", SMALL, 130, 16), C("bwd.gather", SMALL, 5, 129, 1),
    C("bwd.gather", SMALL, 32, 8, 1, 1), C("bwd.gather", SMALL, 65, 13, 0, 1),       # skip_gather at NB = 1 and NB > 1
    C("bwd.gather", SMALL, 64, 65, 0, 1), C("bwd.gather", SMALL, 128, 64, 1, 1),      # two samples per workgroup
    C("bwd.gather", SMALL, 128, 128),      # one sample per workgroup: only past F * d = 8192, where the forward is refused
    # the dense tile: batch < 512, d > 32, or TFRS_DOT_BWD=dense
    C("bwd.dense<1,12>", SMALL, 31, 3, 1), C("bwd.dense<1,12>", SMALL, 78, 32), C("bwd.dense<1,12>", SMALL, 77, 13, 1),
    C("bwd.dense<1,20>", SMALL, 79, 32), C("bwd.dense<1,20>", SMALL, 78, 16, 1), C("bwd.dense<1,20>", SMALL, 101, 21),
    C("bwd.dense<1,20>", SMALL, 100, 8, 1),
    C("bwd.dense<1,33>", SMALL, 102, 32), C("bwd.dense<1,33>", SMALL, 101, 12, 1), C("bwd.dense<1,33>", SMALL, 122, 20, 1),
    C("bwd.dense<2,12>", SMALL, 33, 64, 1), C("bwd.dense<2,12>", SMALL, 64, 33),
    C("bwd.dense<2,20>", SMALL, 96, 48, 1), C("bwd.dense<2,20>", LARGE, 97, 64),
    C("bwd.dense<2,33>", SMALL, 122, 33), C("bwd.dense<2,33>", SMALL, 102, 64, 1),
    C("bwd.dense<4,12>", SMALL, 32, 128, 1), C("bwd.dense<4,12>", SMALL, 64, 65),
    # (more than 3072 pairs at d > 64: F >= 79, where the forward is refused -- the backward is called alone)
    C("bwd.dense<4,20>", SMALL, 79, 100), C("bwd.dense<4,20>", SMALL, 96, 128, 1),
    C("bwd.dense<4,33>", SMALL, 121, 65, 1), C("bwd.dense<4,33>", SMALL, 122, 128),
    C("bwd.dense<1,12>", LARGE, 33, 32, 1, bwd="dense"),
    # the producer / consumer kernel: the default at d < 32, batch >= 512
    C("bwd.pc<12>", LARGE, 31, 3), C("bwd.pc<12>", LARGE, 78, 16), C("bwd.pc<12>", LARGE, 33, 20, 1), C("bwd.pc<12>", LARGE, 3, 32),    # (3 pairs: below a 16-byte load)
    C("bwd.pc<20>", LARGE, 79, 13), C("bwd.pc<20>", LARGE, 100, 8, 1), C("bwd.pc<20>", LARGE, 79, 32, bwd="pc"),
    C("bwd.pc<33>", LARGE, 101, 21, 1), C("bwd.pc<33>", LARGE, 122, 16), C("bwd.pc<33>", LARGE, 102, 32, bwd="pc"),
    # the split-fp16 kernel: d = 32, batch >= 512
    C("bwd.h16<4,3,4>", LARGE, 64, 32, 1), C("bwd.h16<4,3,4>", LARGE, 33, 32), C("bwd.h16<4,3,4>", LARGE, 3, 32, 1),
    C("bwd.h16<7,5,4>", LARGE, 65, 32), C("bwd.h16<7,5,4>", LARGE, 100, 32, 1), C("bwd.h16<7,5,4>", LARGE, 101, 32),
    C("bwd.h16<7,6,4>", LARGE, 101, 32, 1), C("bwd.h16<7,6,4>", LARGE, 110, 32, 1), C("bwd.h16<7,6,4>", LARGE, 111, 32),
    C("bwd.h16<8,8,3>", LARGE, 112, 32), C("bwd.h16<8,8,3>", LARGE, 111, 32, 1), C("bwd.h16<8,8,3>", LARGE, 122, 32, 1),
    # gathered A operand: F = 123 .. 128 (past the dense tile) and TFRS_DOT_BWD=gather
    C("bwd.mfma<8,4>", SMALL, 123, 8), C("bwd.mfma<16,4>", SMALL, 128, 16, 1), C("bwd.mfma<16,4>", LARGE, 123, 13, 1),
    C("bwd.mfma<32,4>", LARGE, 128, 32, 1), C("bwd.mfma<32,4>", SMALL, 123, 20), C("bwd.mfma<64,4>", SMALL, 128, 64, 1),
    C("bwd.mfma<64,4>", SMALL, 124, 33),
    C("bwd.mfma<8,1>", SMALL, 32, 3, 1, bwd="gather"), C("bwd.mfma<8,2>", SMALL, 33, 8, bwd="gather"),
    C("bwd.mfma<8,3>", SMALL, 96, 7, 1, bwd="gather"),
    C("bwd.mfma<16,1>", SMALL, 31, 16, bwd="gather"), C("bwd.mfma<16,2>", SMALL, 64, 13, 1, bwd="gather"),
    C("bwd.mfma<16,3>", SMALL, 65, 12, bwd="gather"),
    C("bwd.mfma<32,1>", SMALL, 32, 21, bwd="gather"), C("bwd.mfma<32,2>", LARGE, 33, 32, 1, bwd="gather"),
    C("bwd.mfma<32,3>", SMALL, 96, 20, 1, bwd="gather"),
    C("bwd.mfma<64,1>", SMALL, 31, 64, 1, bwd="gather"), C("bwd.mfma<64,2>", SMALL, 64, 33, bwd="gather"),
    C("bwd.mfma<64,3>", SMALL, 65, 48, 1, bwd="gather"),
    C("bwd.mfma<128,1>", SMALL, 32, 65, bwd="gather"), C("bwd.mfma<128,2>", SMALL, 33, 128, 1, bwd="gather"),
    C("bwd.mfma<128,2>", SMALL, 64, 100, bwd="gather"),
]

ROUTE_CASES = FWD_ROUTES + BWD_ROUTES

# x 4 bytes past a 16-byte boundary (the scalar loads), out 4 bytes past an 8-byte boundary, odd and even out_dim (the
# float2 or the dword copy-out of the staged kernels), F * d not a multiple of 4: (case, x offset, out offset) in bytes
ALIGNMENT = [
    (C("fwd.mfma<8,1,staged>", SMALL, 6, 8), 4, 0), (C("fwd.mfma<8,1,staged>", SMALL, 6, 8, 1), 0, 4),
    (C("fwd.mfma<8,1,staged>", SMALL, 7, 5, 1), 4, 4), (C("fwd.mfma<8,1,staged>", SMALL, 7, 5), 0, 12),
    (C("fwd.f16x3_direct<16,1,3>", SMALL, 27, 16), 4, 4), (C("fwd.f16x3_direct<16,1,3>", SMALL, 5, 13, 1), 4, 12),
    (C("fwd.f16x3<32,2>", SMALL, 33, 32, fwd="staged"), 4, 4), (C("fwd.f16x3<32,2>", SMALL, 34, 21, 1, fwd="staged"), 12, 4),
    (C("fwd.mfma<64,4,staged>", SMALL, 97, 64), 4, 12), (C("fwd.mfma<64,4,staged>", SMALL, 98, 33, 1), 8, 4),
    (C("fwd.mfma<32,1,direct>", SMALL, 9, 21, 0, 1), 4, 4), (C("fwd.pc<2,4>", LARGE, 33, 32, 1), 0, 4),
    (C("fwd.pc<2,4>", LARGE, 34, 32), 0, 12), (C("bwd.dense<1,12>", SMALL, 27, 13), 4, 4),
    (C("bwd.dense<2,12>", SMALL, 33, 33, 1), 12, 8), (C("bwd.pc<12>", LARGE, 27, 13, 1), 4, 4),
    (C("bwd.h16<4,3,4>", LARGE, 34, 32), 0, 4), (C("bwd.mfma<16,1>", SMALL, 27, 13, bwd="gather"), 4, 12),
    (C("bwd.gather", SMALL, 131, 3), 4, 4),
]

# The persistent kernels at batch = 2 * stride + 5 (stride: the samples of one trip of the grid, from the plan; four per
# workgroup in the two direct-store forward kernels): the second trip of the sample loop and the
# "fetch the next sample under the copy-out" branch, at the smallest F and d of the route: (route, f, d, self, switches)
GRID_STRIDE = [
    ("fwd.mfma<8,1,staged>", 3, 3, 1, {}), ("fwd.mfma<8,2,staged>", 33, 3, 0, {}),
    ("fwd.f16x3<16,1>", 3, 13, 0, {"fwd": "staged"}), ("fwd.f16x3<32,2>", 33, 32, 1, {"fwd": "staged"}),
    ("fwd.pc<2,4>", 33, 32, 0, {}), ("bwd.h16<4,3,4>", 3, 32, 1, {}), ("bwd.pc<12>", 3, 3, 0, {}),
    ("bwd.dense<1,12>", 3, 3, 1, {"bwd": "dense"}), ("bwd.dense<2,12>", 3, 33, 0, {}),
    ("bwd.mfma<8,1>", 3, 3, 1, {"bwd": "gather"}),
    ("fwd.mfma<8,1,direct>", 3, 3, 0, {"skip": 1}), ("fwd.mfma<8,1,direct>", 3, 3, 1, {"stage": "0"}),
    ("fwd.f16x3_direct<16,1,3>", 3, 13, 0, {}), ("fwd.f16x3_direct<32,1,3>", 3, 32, 1, {}),
]


def grid_stride_case(route, f, d, self_i, sw):
  """The case at batch = 2 * stride + 5 and the stride (asked from the plan at a batch larger than any grid)."""
  probe = C(route, 1 << 20, f, d, self_i, **sw)
  stride = samples_per_trip(probe.planned()[probe.direction])
  return C(route, 2 * stride + 5, f, d, self_i, **sw), stride


# the strided entries (the pairs as columns of a wider matrix), D = 16 and D = 32: compared with the contiguous call
STRIDED = [C("fwd.f16x3_direct<16,1,3>", LARGE, 27, 16, strided=1), C("fwd.f16x3_direct<16,2,3>", LARGE, 33, 16, 1, strided=1),
           C("fwd.f16x3_direct<32,1,3>", LARGE, 27, 32, 1, strided=1), C("fwd.pc<2,4>", LARGE, 33, 32, strided=1),
           C("fwd.pc<4,4>", LARGE, 101, 32, strided=1)]
STRIDED_PREFIX = (1, 16)

# the edge of the envelope: (f, d) -> the forward is accepted
ENVELOPE_EDGES = {(64, 128): True, (65, 65): False, (65, 64): True, (130, 30): True, (130, 31): False,
                  (128, 64): True, (128, 65): False, (32, 128): True, (129, 32): False, (31, 129): True, (32, 129): False}
REFUSED_CASES = [(67, 65, 65, 0, 0), (67, 130, 31, 1, 0), (67, 128, 128, 0, 1)]

# one rounding case per route family (gated against the float64 oracle, GATE_DOT of tests/test_ops_gpu.py)
ROUNDING = [C("fwd.mfma<8,2,staged>", SMALL, 33, 5), C("fwd.mfma<128,2,staged>", SMALL, 33, 100, 1),
            C("fwd.mfma<16,1,direct>", SMALL, 27, 13, 0, 1), C("fwd.f16x3<64,2>", SMALL, 33, 48, fwd="staged"),
            C("fwd.f16x3_direct<16,2,3>", SMALL, 33, 13, 1), C("fwd.f16x3_direct<64,3,3>", SMALL, 65, 64),
            C("fwd.f16x3_direct<32,2,3>", SMALL, 33, 32), C("fwd.pc<4,4>", LARGE, 128, 32, 1), C("fwd.gather", SMALL, 130, 16),
            C("bwd.dense<1,12>", SMALL, 27, 13, 1), C("bwd.dense<4,33>", SMALL, 122, 65), C("bwd.pc<20>", LARGE, 79, 13),
            C("bwd.pc<33>", LARGE, 122, 21, 1), C("bwd.h16<8,8,3>", LARGE, 113, 32), C("bwd.mfma<16,4>", SMALL, 123, 13, 1),
            C("bwd.gather", SMALL, 33, 13, 1, 1)]


def all_cases():
  out = list(ROUTE_CASES) + [c for c, _, _ in ALIGNMENT] + STRIDED + ROUNDING
  out += [grid_stride_case(*g)[0] for g in GRID_STRIDE]
  return out


# ------------------------------------------------------------------------------------------ deliberately wrong kernels
def mutant_previous_row_offset(x, self_i):
  """Forward, packed: row i is written where row i - 1 starts."""
  x = np.asarray(x, np.float64)
  g = gram(x)
  f = x.shape[1]
  out = np.zeros((x.shape[0], pairs(f, self_i)))
  for i in range(f):
    off = packed_offset(max(i - 1, 0), self_i)
    for j in range(i + 1 if self_i else i):
      out[:, off + j] = g[:, i, j]
  return out


def mutant_pad_from_next_feature(x, self_i, skip):
  """Forward: the pad columns d .. DP - 1 of a fragment hold the floats that follow in memory (the next feature's
  first columns; zero past the sample) instead of zero."""
  x = np.asarray(x, np.float64)
  b, f, d = x.shape
  dp = padded(d)
  flat = np.concatenate([x.reshape(b, f * d), np.zeros((b, dp))], axis=1)
  xp = np.stack([flat[:, i * d: i * d + dp] for i in range(f)], axis=1)
  return forward64(xp, self_i, skip)


def mutant_stale_sample(ref, grid):
  """Sample b answered from sample b - grid (a stale prefetch / a wrong buffer of the grid-stride loop)."""
  out = np.array(ref, np.float64)
  out[grid:] = ref[: len(ref) - grid]
  return out


def mutant_rows_past_f_stored(x, self_i):
  """Forward, packed: the rows f .. 32 NB - 1 of the last row block are stored too (zeros, since those fragments
  are zero): they land on the head of the next sample's row, and after the last sample in the guard."""
  out = forward64(x, self_i, False)
  f = x.shape[1]
  extra = min(pairs(32 * ((f + 31) // 32), self_i) - pairs(f, self_i), out.shape[1])
  out[1:, :extra] = 0.0
  return out, extra > 0


def mutant_upper_not_zeroed(x):
  x = np.asarray(x, np.float64)
  return gram(x).reshape(x.shape[0], -1)


def mutant_noself_diagonal(x, skip):
  """Forward without self interaction, the diagonal kept: skip_gather shows it in place; packed, G[i][i] lands at
  offset(i) + i = offset(i + 1), the slot of pair (i + 1, 0)."""
  x = np.asarray(x, np.float64)
  g = gram(x)
  f = x.shape[1]
  if skip:
    return np.where(keep_mask(f, True)[None], g, 0.0).reshape(x.shape[0], f * f)
  out = forward64(x, False, False)
  for i in range(f - 1):
    out[:, packed_offset(i + 1, False)] = g[:, i, i]
  return out
