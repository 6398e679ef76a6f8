"""NumPy restatement of ``optimizers.RowWiseAdagrad`` (recommenders_amd/optimizers.py: Adagrad with one accumulator
scalar per table row) in float64 and in float32, and the derived error bounds that the GPU kernels, the torch-op route
and the float32 restatement itself are held to against the float64 restatement on the same float32 inputs.  Duplicates
of a sparse gradient are summed in float32 in the order the route sums them in BOTH variants
(``table_optimizers_restatement.sum_duplicates``), so the summed gradient ``G`` is an input, not an error source.  Test
infrastructure only.

The rule, with ``d`` the row width (csrc/table_rules.h; float32, contraction off, division and ``sqrtf`` correctly
rounded as for the other rules):

    s = (sum_j G_j * G_j) / d ;  acc' = acc + s
    den = sqrt(acc' + eps)            (legacy: sqrt(acc') + eps)
    scale = lr / den ;  w_j' = w_j - scale * G_j

Bounds.  u = 2^-24; E_x is the first-order bound on the error of x, every final bound is 2 * (first-order bound); values
(s, acc', den, ...) are the float64 restatement's.  They hold for ANY order of the d additions inside sum_j: all terms
are non-negative, and a term passes one product and at most d - 1 sums, so its relative error is at most d u; the
division by d (d is exact in float32) adds one rounding:

    E_s     = (d + 1) u s
    E_acc   = E_s + u acc'                                                   (the sum's rounding)
    E_den   = (E_acc + u eps + u (acc' + eps)) / (2 den) + u den             default: eps's rounding, the sum's, the
                                                                             root's derivative 1 / (2 den), its rounding
            = E_acc / (2 sqrt acc') + u sqrt(acc') + u eps + u den           legacy: the root, eps's rounding, the sum's
    E_scale = scale (2 u + E_den / den)                                      lr's rounding, the quotient's
    E_w     = |G_j| E_scale + u |scale G_j| + u |w_j'|                       the product's rounding, the difference's

The float32 restatement sums either sequentially (j ascending) or by a pairwise tree; the kernels use a lane-local
partial per lane and an xor butterfly over the row's lane group, the torch-op route torch's own order.  All are covered.

The band checks bite only if a step moves ``w`` by far more than its bound (``moved_fraction``: more than 100 bounds).
With the cases of ``table_optimizers_restatement.sparse_cases`` at ``learning_rate = 256`` at least 0.99 of the elements
with a non-zero gradient do (0.97 at 64, only 0.89 at 16): ``LR = 256`` and the tests assert >= 0.95.
"""

import ctypes

import numpy as np

from recommenders_amd import _lib

U = 2.0 ** -24
LR = 256.0


def hyper(legacy=False, learning_rate=LR, epsilon=1e-7, initial_accumulator_value=0.1):
  return dict(learning_rate=learning_rate, epsilon=epsilon, legacy=legacy,
              initial_accumulator_value=initial_accumulator_value)


def _sum_squares(g, order):
  """float32 sum over the last axis of g * g: ``sequential`` (j ascending) or a ``pairwise`` tree."""
  sq = g * g
  if order == "sequential":
    total = np.zeros(sq.shape[:-1], dtype=np.float32)
    for j in range(sq.shape[-1]):
      total = total + sq[..., j]
    return total
  while sq.shape[-1] > 1:
    if sq.shape[-1] % 2:
      sq = np.concatenate([sq, np.zeros(sq.shape[:-1] + (1,), dtype=np.float32)], axis=-1)
    sq = sq[..., 0::2] + sq[..., 1::2]
  return sq[..., 0]


def update(w, acc, g, hp, dtype, order="sequential", sum_sq=None):
  """One step on ``w [r, d]``, ``acc [r]``, ``g [r, d]`` (the summed gradient) in ``dtype`` arithmetic.  ``sum_sq``: the
  rows' ``sum_j g_j * g_j`` taken as given in place of ``order`` -- the kernels' own orders are restated in
  tests/optimizer_handbuilt.py (``sum_squares_kernel_order``, ``sum_squares_rowscan_order``).  Returns a dict: w, acc and
  the intermediates the bounds need."""
  t = np.dtype(dtype).type
  w, acc, g = (np.asarray(x, dtype=dtype) for x in (w, acc, g))
  d = g.shape[-1]
  if sum_sq is not None:
    sum_sq = np.asarray(sum_sq)
    assert sum_sq.dtype == dtype and sum_sq.shape == g.shape[:-1]
  elif dtype == np.float64:
    sum_sq = (g * g).sum(axis=-1)
  else:
    sum_sq = _sum_squares(g, order)
  s = sum_sq / t(d)
  acc2 = acc + s
  eps = t(hp["epsilon"])
  den = np.sqrt(acc2) + eps if hp["legacy"] else np.sqrt(acc2 + eps)
  scale = t(hp["learning_rate"]) / den
  step = scale[..., None] * g
  out = dict(w=w - step, acc=acc2, s=s, den=den, scale=scale, step=step, eps=eps, legacy=bool(hp["legacy"]), d=d)
  assert out["w"].dtype == dtype and out["acc"].dtype == dtype
  return out


def bounds(ref64, g):
  """The module docstring's bounds from the float64 step ``ref64``: dict with ``w`` and ``accumulator``."""
  g = np.abs(np.asarray(g, dtype=np.float64))
  d, s, acc2, den, scale, eps = ref64["d"], ref64["s"], ref64["acc"], ref64["den"], ref64["scale"], ref64["eps"]
  e_s = (d + 1) * U * s
  e_acc = e_s + U * acc2
  if ref64["legacy"]:
    root = np.sqrt(acc2)
    e_den = e_acc / (2 * root) + U * root + U * eps + U * den
  else:
    e_den = (e_acc + U * eps + U * (acc2 + eps)) / (2 * den) + U * den
  e_scale = scale * (2 * U + e_den / den)
  e_w = g * e_scale[..., None] + U * np.abs(ref64["step"]) + U * np.abs(ref64["w"])
  return dict(w=2 * e_w, accumulator=2 * e_acc)


def check_step(got_w, got_acc, ref64, g, label=""):
  """Asserts the bounds for one step: ``got_*`` (float32 results) against ``ref64`` (``update(..., np.float64)`` from
  the same float32 state and gradient).  Returns the observed fraction of each budget."""
  b = bounds(ref64, g)
  used = {}
  for key, got, ref in (("w", got_w, ref64["w"]), ("accumulator", got_acc, ref64["acc"])):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape == b[key].shape, (key, got.dtype, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    used[key] = float((err / np.maximum(b[key], 1e-300)).max()) if err.size else 0.0
    assert (err <= b[key]).all(), f"{label} {key}: {used[key]:.3f} of the bound"
  return used


def moved_fraction(ref64, g, w_before):
  """Fraction of the elements with a non-zero gradient whose float64 step moves ``w`` by more than 100 x its bound."""
  g = np.asarray(g)
  nonzero = g != 0
  if not nonzero.any():
    return 1.0
  moved = np.abs(ref64["w"] - np.asarray(w_before, dtype=np.float64)) > 100 * bounds(ref64, g)["w"]
  return float(moved[nonzero].mean())


def row_accumulator(case):
  """The per-row accumulator a sparse case of ``table_optimizers_restatement.sparse_cases`` starts from: column 0 of its
  per-element one (0.025 .. 0.225)."""
  return np.ascontiguousarray(case["acc"][:, 0])


def c_entry_argument_cases(lib):
  """(call, return code, text of the message): shared with the GPU tests.  NULL or fake device pointers throughout."""
  fake = ctypes.c_void_p(256)

  def sparse(table=fake, accum=fake, grad=fake, ids=fake, n=4, d=8, vocab=10, mode=1, rowscan=0, ws=fake, ws_bytes=1 << 30,
             eps=1e-7):
    return lambda: lib.tfrs_rowwise_adagrad_sparse(grad, ids, 1, n, d, vocab, table, accum, 0.1, None, eps, mode, rowscan,
                                                   ws, ws_bytes, None)

  def dense(param=fake, accum=fake, grad=fake, rows=4, d=8, mode=1, eps=1e-7):
    return lambda: lib.tfrs_rowwise_adagrad_dense(param, accum, grad, rows, d, 0.1, None, eps, mode, None)

  return [
      (sparse(table=None), _lib.TFRS_EINVAL, "NULL pointer"),
      (sparse(accum=None), _lib.TFRS_EINVAL, "NULL pointer"),
      (sparse(grad=None), _lib.TFRS_EINVAL, "NULL pointer"),
      (sparse(d=0), _lib.TFRS_EINVAL, "bad shape"),
      (sparse(n=-1), _lib.TFRS_EINVAL, "bad shape"),
      (sparse(vocab=1 << 33), _lib.TFRS_EINVAL, "32 bits"),
      (sparse(mode=0), _lib.TFRS_EINVAL, "mode must be"),
      (sparse(mode=3), _lib.TFRS_EINVAL, "mode must be"),
      (sparse(eps=-1.0), _lib.TFRS_EINVAL, "non-negative"),
      (sparse(d=300, rowscan=1), _lib.TFRS_EINVAL, "row-scan"),
      (sparse(ws=None), _lib.TFRS_EINVAL, "NULL workspace"),
      (sparse(ws_bytes=lib.tfrs_table_update_workspace_bytes(4, 0) - 1), _lib.TFRS_ENOMEM, "workspace too small"),
      (dense(param=None), _lib.TFRS_EINVAL, "NULL pointer"),
      (dense(d=0), _lib.TFRS_EINVAL, "bad shape"),
      (dense(rows=-1), _lib.TFRS_EINVAL, "bad shape"),
      (dense(mode=7), _lib.TFRS_EINVAL, "mode must be"),
  ]
