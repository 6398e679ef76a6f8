"""Hand-built tensors and rows for the optimizer kernels (csrc/table_update.hip, csrc/clippy.hip and the rule kernels at
the end of csrc/sparse_update.hip): every builder returns the data together with a description of what it planted, so a
test chooses what the kernels see -- a tensor that ends exactly on a block, an empty tensor between two others, one
operand 4 bytes off, the only clipped element of a tensor in a chosen block, a row wider than its lane group -- instead
of taking what a random draw produces.  tests/test_optimizer_handbuilt_host.py proves every planted property again from
the arrays alone; tests/test_optimizer_layout_gpu.py compares the kernels with the restatements bit for bit.

Three things are restated here that no other file restates:

  * the FUSED variants of the SGD / Adam / Ftrl rules: ``table_optimizers_restatement.update(..., np.float32)`` with every
    ``a * b +- c`` that a compiler could contract inside the rule's ``apply`` turned into one rounding.  Their only use is
    the host proof that the rule cases tell a contracted kernel from the contract of csrc/table_rules.h;
  * the order in which the RowWiseAdagrad kernels add the squares of a row (``sum_squares_kernel_order``,
    ``sum_squares_rowscan_order``; csrc/table_rules.h);
  * the walk of the dense multi-tensor kernels over ``first_block[]`` and their float4 / scalar choice per block
    (``dense_blocks``).

Pure numpy, no GPU access.  Test infrastructure only."""

import numpy as np

from tests import clippy_restatement as crs
from tests import table_optimizers_restatement as rs

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
WRAPS_TO_3 = 2 ** 32 + 3  # an int64 id that a truncation to 32 bits would turn into the valid id 3
MIN_NORMAL = 2.0 ** -126

GUARD = 8                 # sentinel floats in front of, between and behind the tensors of a packed buffer
SENTINEL = F32(-7.25e8)


def bits(a):
  """The float32 array's bit patterns (a comparison that sets -0 apart from +0)."""
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fma(a, b, c):
  """``a * b + c`` with one rounding, emulated through float64 (the product of two float32 is exact there)."""
  a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
  return (a * b + c).astype(np.float32)


# ---- the rules: hyper-parameters, intermediates, fused variants ----------------------------------------------------------
RULE_NAMES = tuple(sorted(rs.RULES))
RULE_INDEX = {"SGD": 0, "Adam": 1, "Ftrl": 2}       # the `rule` argument of the C entries
SGD_LR = 0.3                                        # not a power of two: lr * g rounds, so w - lr * g can show a fusion


def rule_hyper(name):
  """(kind, hyper-parameters) of ``rs.RULES[name]``, SGD at a learning rate that is no power of two."""
  kind, hp = rs.RULES[name]
  hp = dict(hp)
  if kind == "SGD":
    hp["learning_rate"] = SGD_LR
  return kind, hp


def rule_hyper_floats(kind, hp):
  """The 8 ``hyper_h`` floats of the C entries (csrc/table_rules.h), computed in double as ``optimizers.py`` does and
  rounded to float32 once."""
  if kind == "SGD":
    h = [hp["learning_rate"]]
  elif kind == "Adam":
    h = [1.0 - hp["beta_1"], 1.0 - hp["beta_2"], hp["epsilon"]]
  else:
    full = dict(rs._FTRL_DEFAULTS, **hp)
    lr = full["learning_rate"]
    h = [lr, full["l1_regularization_strength"], 2.0 * (full["l2_regularization_strength"] + full["beta"] / (2.0 * lr)),
         2.0 * full["l2_shrinkage_regularization_strength"], full["learning_rate_power"]]
  return np.asarray(h + [0.0] * (8 - len(h)), dtype=np.float32)


def _ftrl_constants(hp):
  full = dict(rs._FTRL_DEFAULTS, **hp)
  lr, l1 = F32(full["learning_rate"]), F32(full["l1_regularization_strength"])
  k = F32(2.0 * (full["l2_regularization_strength"] + full["beta"] / (2.0 * full["learning_rate"])))
  c = F32(2.0 * full["l2_shrinkage_regularization_strength"])
  return lr, l1, k, c, full["learning_rate_power"] != 0.0


def rule_intermediates(kind, w, slots, g, hp, alpha=None):
  """The float32 step of ``rs.update`` once more with EVERY intermediate kept (the products ``g * g``, ``lr * g``, ...
  included): dict with ``w``, ``slots`` and ``all``, the list of the intermediates in the order they are computed."""
  w, g = np.asarray(w, np.float32), np.asarray(g, np.float32)
  slots = [np.asarray(s, np.float32) for s in slots]
  if kind == "SGD":
    step = F32(hp["learning_rate"]) * g
    w2 = w - step
    return dict(w=w2, slots=[], all=[step, w2])
  if kind == "Adam":
    m, v = slots
    c1, c2, eps, a = F32(1.0 - hp["beta_1"]), F32(1.0 - hp["beta_2"]), F32(hp["epsilon"]), F32(alpha)
    gm = g - m
    t1 = gm * c1
    m2 = m + t1
    gg = g * g
    gv = gg - v
    t2 = gv * c2
    v2 = v + t2
    root = np.sqrt(v2)
    den = root + eps
    ma = m2 * a
    step = ma / den
    w2 = w - step
    return dict(w=w2, slots=[m2, v2], all=[gm, t1, m2, gg, gv, t2, v2, root, den, ma, step, w2])
  lr, l1, k, c, root = _ftrl_constants(hp)
  n, lin = slots
  cw = c * w
  gp = g + cw
  gg = g * g
  n2 = n + gg
  pn2 = np.sqrt(n2) if root else np.ones_like(n2)
  pn = np.sqrt(n) if root else np.ones_like(n)
  diff = pn2 - pn
  quot = diff / lr
  s = quot * w
  inner = gp - s
  lin2 = lin + inner
  ql = pn2 / lr
  q = ql + k
  clip = np.minimum(np.maximum(lin2, -l1), l1)
  num = clip - lin2
  w2 = num / q
  return dict(w=w2, slots=[n2, lin2], lin2=lin2,
              all=[cw, gp, gg, n2, pn2, pn, diff, quot, s, inner, lin2, ql, q, clip, num, w2])


def fused_update(kind, w, slots, g, hp, alpha=None):
  """``rs.update(..., np.float32)`` with every contractible ``a * b +- c`` of the rule's ``apply`` rounded once:

    SGD   w - lr * g
    Adam  m + (g - m) * c1;  g * g - v;  v + (...) * c2              (m * alpha / den is a product and a QUOTIENT: no fusion)
    Ftrl  g + c * w;  n + g * g;  g' - ((P' - P) / lr) * w           (P' / lr + k: a quotient, no fusion)

  Returns a dict: w, slots."""
  w, g = np.asarray(w, np.float32), np.asarray(g, np.float32)
  slots = [np.asarray(s, np.float32) for s in slots]
  if kind == "SGD":
    return dict(w=fma(-F32(hp["learning_rate"]), g, w), slots=[])
  if kind == "Adam":
    m, v = slots
    c1, c2, eps, a = F32(1.0 - hp["beta_1"]), F32(1.0 - hp["beta_2"]), F32(hp["epsilon"]), F32(alpha)
    m2 = fma(g - m, c1, m)
    v2 = fma(fma(g, g, -v), c2, v)
    return dict(w=w - m2 * a / (np.sqrt(v2) + eps), slots=[m2, v2])
  lr, l1, k, c, root = _ftrl_constants(hp)
  n, lin = slots
  gp = fma(c, w, g)
  n2 = fma(g, g, n)
  pn2 = np.sqrt(n2) if root else np.ones_like(n2)
  pn = np.sqrt(n) if root else np.ones_like(n)
  lin2 = lin + fma(-((pn2 - pn) / lr), w, gp)
  q = pn2 / lr + k
  return dict(w=(np.minimum(np.maximum(lin2, -l1), l1) - lin2) / q, slots=[n2, lin2])


def rule_weights(rng, shape):
  """About 1e-3 N(0, 1): of the step's own magnitude, so the last bits of ``w`` depend on how the step was rounded."""
  return (rng.normal(size=shape) * 1e-3).astype(np.float32)


def rule_gradients(rng, shape):
  """About 3e-3 N(0, 1); from 3 elements on a few exact zeros of both signs, from 5 elements on a few entries 10^4 x
  larger."""
  g = (rng.normal(size=shape) * 3e-3).astype(np.float32)
  flat = g.reshape(-1)
  if flat.size >= 3:
    at = rng.integers(0, flat.size, size=max(2, flat.size // 50))
    flat[at[0::2]] = 0.0
    flat[at[1::2]] = -0.0
  if flat.size >= 5:
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 1000))] *= F32(1e4)
  return g


def rule_start(name, rng, w):
  """The slots rule ``name`` starts from at weights ``w`` and the step number t of the first step the test takes: Adam's
  after ONE restated step from zero (t = 2), Ftrl's accumulator at 0.5 .. 2 x 1e-5 with the consistent ``linear``."""
  kind, hp = rule_hyper(name)
  if kind == "Adam":
    out = rs.update("Adam", w, [np.zeros_like(w), np.zeros_like(w)], rule_gradients(rng, w.shape), hp, np.float32,
                    alpha=F32(rs.adam_alpha(hp, 1)))
    return out["slots"], 2
  if kind == "Ftrl":
    n = (rng.uniform(0.5, 2.0, size=w.shape) * 1e-5).astype(np.float32)
    return [n, rs.ftrl_consistent_linear(hp, w, n).astype(np.float32)], 1
  return [], 1


def rule_alpha(name, t):
  """Adam's step size at step ``t`` as the float32 the test hands the kernels (``None`` for the other rules)."""
  kind, hp = rule_hyper(name)
  return F32(rs.adam_alpha(hp, t)) if kind == "Adam" else None


_RULE_CASES = {}


def rule_case(name, n, steps=2, seed=0):
  """The rule case of ``name`` on ``n`` elements: dict with kind, hp, w, slots, grads (one per step), alphas (one per
  step) and ``ref``, the restated float32 steps (``rs.update``) in sequence -- computed once and read-only."""
  key = (name, n, steps, seed)
  if key not in _RULE_CASES:
    kind, hp = rule_hyper(name)
    rng = np.random.default_rng(90_000 + 1000 * RULE_NAMES.index(name) + 7 * seed + n % 997)
    w = rule_weights(rng, (n,))
    slots, t0 = rule_start(name, rng, w)
    grads = [rule_gradients(rng, (n,)) for _ in range(steps)]
    alphas = [rule_alpha(name, t0 + s) for s in range(steps)]
    ref, cw, cs = [], w, slots
    for g, a in zip(grads, alphas):
      out = rs.update(kind, cw, cs, g, hp, np.float32, alpha=a)
      ref.append(out)
      cw, cs = out["w"], out["slots"]
    for a in [w] + list(slots) + grads:
      a.setflags(write=False)
    _RULE_CASES[key] = dict(name=name, kind=kind, hp=hp, w=w, slots=slots, grads=grads, alphas=alphas, ref=ref)
  return _RULE_CASES[key]


# ---- the dense multi-tensor layout -----------------------------------------------------------------------------------------
DENSE_BLOCK = 256 * 16     # kDenseUpdatePerBlock / kClippyPerBlock
DENSE_SIZES = (0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1027)
# exactly 32 tensors: an empty one first, two consecutive empty ones in the middle, an empty one last
LIST_32 = (0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 0, 0, 8192, 8193, 3 * 4096 + 1027, 1, 4096, 5, 3, 4097, 4,
           1, 8192, 3, 5, 4096, 4, 1, 4095, 3, 5, 4, 0)
OPERANDS = ("p", "s0", "s1", "g")
ALIGNMENTS = ("aligned", "all_off", "p_off", "s0_off", "s1_off", "g_off")


def dense_lists():
  """name -> tuple of tensor sizes: every size of DENSE_SIZES alone (``n0`` is a call that launches nothing), the list of
  32 and an all-empty list."""
  out = {f"n{n}": (n,) for n in DENSE_SIZES}
  out["list32"] = LIST_32
  out["all_empty"] = (0, 0, 0)
  return out


def operand_off(alignment, operand):
  """Whether ``operand``'s tensors start 4 bytes off a 16-byte boundary under ``alignment``."""
  assert alignment in ALIGNMENTS and operand in OPERANDS
  return alignment == "all_off" or alignment == operand + "_off"


def pack(sizes, off):
  """Where the tensors of one operand go in ONE flat buffer whose start is 16-byte aligned: GUARD or more sentinel
  floats in front of, between and behind them, every tensor at a multiple of 4 floats (``off``: one float further).
  Returns (offset per tensor, ``None`` for an empty one -- it gets a NULL pointer --, length of the buffer)."""
  offsets, cursor = [], 0
  for n in sizes:
    start = -(-(cursor + GUARD) // 4) * 4 + (1 if off else 0)
    offsets.append(start if n else None)
    if n:
      cursor = start + n
  return offsets, -(-(cursor + GUARD) // 4) * 4 + 4


def packed(sizes, off, arrays):
  """The flat buffer of ``pack`` with ``arrays`` in place and the sentinel everywhere else."""
  offsets, total = pack(sizes, off)
  flat = np.full((total,), SENTINEL, dtype=np.float32)
  for o, n, a in zip(offsets, sizes, arrays):
    if n:
      assert a.shape == (n,) and a.dtype == np.float32
      flat[o:o + n] = a
  return flat


def tensor_walk(first_block, ntensors, block):
  """The kernels' ``while (k + 1 < ntensors && block >= first_block[k + 1]) ++k``: (k, number of steps that passed an
  EMPTY tensor)."""
  k, over_empty = 0, 0
  while k + 1 < ntensors and block >= first_block[k + 1]:
    over_empty += int(first_block[k + 1] == first_block[k])
    k += 1
  return k, over_empty


def dense_blocks(sizes, off_by_operand):
  """The launch of a dense multi-tensor kernel restated from (sizes, alignment): dict with ``first_block`` (ntensors + 1
  entries) and ``blocks``, one entry per block: (tensor k the walk ends at, the block's first element ``base`` inside
  the tensor, ``float4`` or ``scalar``, steps of the walk over an empty tensor).  ``off_by_operand``: one bool per
  operand the kernel ORs into its alignment test."""
  first_block, blocks = [0], []
  for n in sizes:
    first_block.append(first_block[-1] + -(-n // DENSE_BLOCK))
  aligned = not any(off_by_operand)
  for b in range(first_block[-1]):
    k, over_empty = tensor_walk(first_block, len(sizes), b)
    base = (b - first_block[k]) * DENSE_BLOCK
    path = "float4" if aligned and base + DENSE_BLOCK <= sizes[k] else "scalar"
    blocks.append((k, base, path, over_empty))
  return dict(first_block=first_block, blocks=blocks)


def list_rule_case(name, sizes, steps=2):
  """The rule case of ``name`` on every tensor of ``sizes`` (tensors of one size at different places of a list hold
  different data): (case of the concatenation, list of slices)."""
  total = int(sum(sizes))
  case = rule_case(name, total, steps, seed=len(sizes))
  cuts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  return case, [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


# ---- exact cases for the kernels compiled with contraction on ------------------------------------------------------------------
# (mode, eps): eps = 0 in both modes; an eps != 0 per mode at which THAT mode's denominator is a power of two
ADAGRAD_EXACT = ((1, 0.0), (2, 0.0), (1, 3.0 * 2.0 ** -8), (2, 2.0 ** -4))
ADAGRAD_LR = 2.0 ** -3


def adagrad_exact_case(n, mode, eps, seed=0):
  """``n`` elements on which every operation of the dense Adagrad update is exact.

  eps == 0: g = +-2^e (e in -6 .. -2), acc = (m^2 - 1) g^2 with m in {1, 2, 4, 8}, w a multiple of 2^-6 = lr / 8 in
  [-1, 1]: acc' = m^2 g^2, the root is m |g|, the step +-lr / m; every 17th element has g = +-0 over acc = 2^-4 (no step).
  eps != 0: (m, |g|) in {(1, 2^-4), (2, 2^-5), (4, 2^-6), (8, 2^-7)}, so sqrt(acc') = 2^-4 everywhere; mode 1 with
  eps = 3 * 2^-8: sqrt(2^-8 + 3 * 2^-8) = 2^-3; mode 2 with eps = 2^-4: 2^-4 + 2^-4 = 2^-3; the step is +-g.  Under the
  OTHER mode the same inputs give a denominator that is no power of two (the host test asserts different results).
  Returns a dict: w, acc, g, lr, eps, mode."""
  rng = np.random.default_rng(40_000 + 100 * mode + int(eps != 0.0) * 10 + seed + n % 991)
  m = 2.0 ** rng.integers(0, 4, size=n)
  sign = rng.choice([-1.0, 1.0], size=n)
  if eps == 0.0:
    g = sign * 2.0 ** rng.integers(-6, -1, size=n)
  else:
    g = sign * 2.0 ** -4 / m
  acc = (m * m - 1.0) * g * g
  if eps == 0.0:
    acc[3::17] = 2.0 ** -4
    g[3::17] = np.where(sign[3::17] > 0, 0.0, -0.0)
  w = rng.integers(-64, 65, size=n) * 2.0 ** -6
  return dict(w=w.astype(np.float32), acc=acc.astype(np.float32), g=g.astype(np.float32), lr=ADAGRAD_LR, eps=eps,
              mode=mode)


def adagrad_eval(w, acc, g, lr, eps, mode, dtype, fused=False):
  """``acc' = acc + g * g;  w' = w - lr * g / denom(acc')`` (csrc/table_rules.h: adagrad_denom) in ``dtype`` arithmetic
  on the float32 inputs; ``fused`` (float32 only): acc' with one rounding.  Returns (w', acc')."""
  t = np.dtype(dtype).type
  lr, eps = t(F32(lr)), t(F32(eps))
  if fused:
    acc2 = fma(g, g, acc)
    w, g = np.asarray(w, np.float32), np.asarray(g, np.float32)
  else:
    w, acc, g = (np.asarray(x, np.float32).astype(dtype) for x in (w, acc, g))
    acc2 = acc + g * g
  den = np.sqrt(acc2) + eps if mode == 2 else np.sqrt(acc2 + eps)
  return w - lr * g / den, acc2


CLIPPY_MODES = (0, 1, 2)
CLIPPY_MAX_J = 7


def clippy_exact_hyper(mode):
  """Keyword arguments of ``clippy_restatement.update`` for the exact cases: every threshold a power of two, eps = 0."""
  if mode == 2:
    hp = dict(learning_rate=2.0 ** -3, variable_relative_threshold=2.0 ** -3, accumulator_relative_threshold=2.0 ** -10,
              absolute_threshold=2.0 ** -12)
  else:
    hp = dict(learning_rate=2.0 ** -6, variable_relative_threshold=2.0 ** -3, accumulator_relative_threshold=2.0 ** -3,
              absolute_threshold=2.0 ** -3)
  return dict(hp, epsilon=0.0, **crs.MODES[mode])


def plant_positions(n):
  """name -> index of the places a tensor of ``n`` elements offers for its only clipped element: ``first``; ``last_full``,
  the last element of the last full block; ``tail``, inside the ending block (neither its first nor its last element
  where it has three); ``last``, element n - 1."""
  out = {}
  full = n // DENSE_BLOCK * DENSE_BLOCK
  if n >= 1:
    out["first"] = 0
  if full:
    out["last_full"] = full - 1
  if n - full >= 3:
    out["tail"] = full + (n - full) // 2
  if n >= 2:
    out["last"] = n - 1
  return out


def clippy_exact_tensor(n, mode, plant=None, seed=0):
  """One tensor of the exact Clippy case: (w, acc, g).  ``plant``: ``None`` (no element is clipped: factor exactly 1) or
  (index, j), 1 <= j <= 7: that element's |delta| is 2^j times its allowed change, so the factor is exactly 2^-j.

  Modes 0 and 1 (lr = 2^-6, thresholds 2^-3): acc in {4, 16}, so pre = 1 / sqrt(acc) in {1/2, 1/4}; g in +-{1, 1/2,
  1/4} and a few +-0; |w| = k / 16, k in 4 .. 12.  |delta| <= 2^-7 is below the allowed change >= 2^-5 + 2^-3.  The
  planted element: acc = 4, |w| = 1/2, g = +-2^(j + 5): allowed change 2^-4 + 2^-4 + 2^-3 = 2^-2, |delta| = 2^(j - 2).
  Mode 2 (lr = 2^-3, thresholds 2^-3, 2^-10, 2^-12): g = +-2^a (a in -3 .. 0) over acc = 63 g^2, so acc' = 64 g^2,
  pre = 1 / (8 |g|) and |delta| = 2^-6 below |w| / 8 >= 2^-5; a few +-0 over acc = 4.  The planted element: acc = 0,
  g = +-4 (pre = 1/4, |delta| = lr), |w| = 2^-8 (2^(8 - j) - 1): allowed change 2^-11 (2^(8 - j) - 1) + 2^-12 + 2^-12 =
  2^(-3 - j).  All sums stay inside 24 bits (the host test evaluates in float64, float32 and with fusions)."""
  rng = np.random.default_rng(60_000 + 1000 * mode + 13 * seed + n % 983)
  sign = rng.choice([-1.0, 1.0], size=n)
  w = rng.choice([-1.0, 1.0], size=n) * rng.integers(4, 13, size=n) / 16.0
  zero = np.zeros(n, bool)
  zero[5::23] = True
  if mode == 2:
    g = sign * 2.0 ** rng.integers(-3, 1, size=n)
    acc = 63.0 * g * g
  else:
    g = sign * 2.0 ** rng.integers(-2, 1, size=n)
    acc = 4.0 ** rng.integers(1, 3, size=n)
  acc[zero] = 4.0
  g[zero] = np.where(sign[zero] > 0, 0.0, -0.0)
  if plant is not None:
    at, j = plant
    assert 0 <= at < n and 1 <= j <= CLIPPY_MAX_J
    if mode == 2:
      w[at], acc[at], g[at] = sign[at] * 2.0 ** -8 * (2.0 ** (8 - j) - 1.0), 0.0, -sign[at] * 4.0
    else:
      w[at], acc[at], g[at] = sign[at] * 0.5, 4.0, sign[at] * 2.0 ** (j + 5)
  return w.astype(np.float32), acc.astype(np.float32), g.astype(np.float32)


def clippy_fused(w, acc, g, hp):
  """The float32 Clippy step as csrc/clippy.h writes it, with its explicit fused multiply-adds AND the contractible
  ``w - delta * factor`` rounded once: dict of w, acc, factor."""
  w, acc, g = (np.asarray(x, np.float32) for x in (w, acc, g))
  mode = crs._mode(hp)
  lr, eps = F32(hp["learning_rate"]), F32(hp["epsilon"])
  var_rel, acc_rel, abs_thr = (F32(hp[k]) for k in ("variable_relative_threshold", "accumulator_relative_threshold",
                                                    "absolute_threshold"))
  e_acc = fma(g, g, acc) if mode == 2 else acc
  pre = F32(1.0) / np.sqrt(e_acc + eps)
  delta = lr * g * pre
  maxd = np.abs(w) * var_rel + pre * acc_rel + abs_thr
  ad = np.abs(delta)
  clipped = ad > maxd
  factor = F32(min(1.0, (maxd[clipped] / ad[clipped]).min())) if clipped.any() else F32(1.0)
  new_w = fma(-delta, factor, w)
  if mode != 2:
    u = g * factor if mode == 1 else g
    e_acc = fma(u, u, e_acc)
  return dict(w=new_w, acc=e_acc, factor=factor)


# the 32-tensor list's planted tensors: index -> (place, j); every other tensor's factor is exactly 1
LIST_32_PLANTS = {1: ("first", 3), 7: ("last_full", 6), 11: ("last_full", 1), 12: ("last", 7), 13: ("tail", 2),
                  15: ("first", 5), 30: ("last", 4)}


def clippy_lists():
  """name -> (sizes, plants): plants[k] is ``None`` or (index, j).  Every size alone with its only clipped element at
  each place the size offers, every size alone without one, the list of 32 with LIST_32_PLANTS, the all-empty list."""
  out = {}
  count = 0
  for n in DENSE_SIZES:
    out[f"n{n}.none"] = ((n,), [None])
    for place, at in plant_positions(n).items():
      out[f"n{n}.{place}"] = ((n,), [(at, 1 + count % CLIPPY_MAX_J)])
      count += 1
  plants = [None] * 32
  for k, (place, j) in LIST_32_PLANTS.items():
    plants[k] = (plant_positions(LIST_32[k])[place], j)
  out["list32"] = (LIST_32, plants)
  out["all_empty"] = ((0, 0, 0), [None] * 3)
  return out


# ---- sparse cases --------------------------------------------------------------------------------------------------------
SPARSE_DIMS = (1, 3, 4, 8, 200, 256)
SPARSE_DIMS_SORTED = SPARSE_DIMS + (260,)
ROWSCAN_VOCAB = 37          # vocab % 4 != 0: the last workgroup of the row scan has dead waves
SORTED_VOCAB = 1000
HOT_ID, HOT_COUNT = 3, 40   # more occurrences than a piece of 32 positions


def sparse_ids(vocab, id_dtype, seed=0):
  """At most 400 hand-built ids: 300 drawn ones with duplicates, HOT_ID 40 times, ids 0 and vocab - 1, a pair of
  ``zero_pair`` (the test plants x and -x there), and -1, vocab, INT32_MAX (int64 lists: 2^32 + 3 too) three times each
  at scattered places.  The rows of ``untouched`` and ``zero_pair`` are never drawn.  Returns a dict: ids, vocab,
  zero_pair, untouched."""
  rng = np.random.default_rng(70_000 + vocab + seed)
  untouched = np.array([1, vocab // 2, vocab - 2])
  zero_pair = 5
  allowed = np.setdiff1d(np.arange(vocab), np.r_[untouched, zero_pair])
  ids = np.r_[allowed[rng.integers(0, allowed.size, size=300)], [HOT_ID] * HOT_COUNT, [0, vocab - 1],
              [zero_pair, zero_pair]].astype(np.int64)
  ids = ids[rng.permutation(ids.size)]
  invalid = [-1, vocab, INT32_MAX] + ([WRAPS_TO_3] if np.dtype(id_dtype) == np.int64 else [])
  where = np.linspace(0, ids.size, num=3 * len(invalid), endpoint=False).astype(np.int64)
  ids = np.insert(ids, where, np.asarray(invalid * 3, np.int64))
  assert ids.size <= 400
  return dict(ids=ids.astype(id_dtype), vocab=vocab, zero_pair=zero_pair, untouched=untouched)


def sparse_rows(case, d, seed=0):
  """Gradient rows of the rule cases' scale for the id list ``case``; the two occurrences of ``zero_pair`` get x, -x."""
  rng = np.random.default_rng(71_000 + 31 * seed + d)
  rows = rule_gradients(rng, (case["ids"].size, d))
  a, b = np.flatnonzero(case["ids"].astype(np.int64) == case["zero_pair"])
  rows[b] = -rows[a]
  return rows


def unique_ids(vocab, id_dtype, seed=0):
  """Every row of the table exactly once, in a scrambled order (no duplicate sum: all routes see the same gradient)."""
  return np.random.default_rng(72_000 + vocab + seed).permutation(vocab).astype(id_dtype)


# ---- RowWiseAdagrad ------------------------------------------------------------------------------------------------------
ROWWISE_DIMS = (1, 2, 3, 4, 5, 63, 64, 65, 200, 256, 257, 260, 520)
ROWWISE_ROWS = (1, 5, 67)
ROWWISE_GRID_CAP = 256 * 64        # blocks of rowwise_adagrad_dense_kernel before it grid-strides
ROWWISE_LR = 0.003                # scale = lr / den is about 1, so the step is of the weights' own magnitude


def group_lanes(d, vec):
  """Lanes of a row's group: the power of two >= d / vec, at most 64."""
  per_row = d // vec
  lanes = 1
  while lanes < 64 and lanes < per_row:
    lanes *= 2
  return lanes


def rowwise_path(d, aligned):
  """(VEC, REREAD) of the sorted route / the dense kernel at width ``d``: the float4 path where d % 4 == 0 and the
  operands are 16-byte aligned; REREAD where a row has more chunks than 64 lanes."""
  vec = 4 if d % 4 == 0 and aligned else 1
  return vec, d // vec > 64


def _butterfly(partial):
  """x += x of lane ^ offset with the offsets L / 2, L / 4, ..., 1: every lane ends with the same bits."""
  lanes = partial.shape[-1]
  lane = np.arange(lanes)
  o = lanes >> 1
  while o:
    partial = partial + partial[..., lane ^ o]
    o >>= 1
  assert (bits(partial) == bits(partial[..., :1])).all()
  return partial[..., 0]


def _lane_partials(g, vec, lanes):
  """Lane l adds the squares of the chunks l, l + L, ... (ascending; the ``vec`` elements of a chunk ascending) to a
  partial that starts at +0.  (A row padded with +0 elements: partial + 0 * 0 keeps the partial's bits, which are never
  those of -0.)"""
  g = np.asarray(g, dtype=np.float32)
  rows, d = g.shape
  rounds = -(-d // (lanes * vec))
  padded = np.zeros((rows, rounds * lanes * vec), dtype=np.float32)
  padded[:, :d] = g
  padded = padded.reshape(rows, rounds, lanes, vec)
  partial = np.zeros((rows, lanes), dtype=np.float32)
  for r in range(rounds):
    for e in range(vec):
      x = padded[:, r, :, e]
      partial = partial + x * x
  return partial


def sum_squares_kernel_order(g, vec):
  """float32 ``sum_j g_j * g_j`` of every row of ``g [rows, d]`` in the order of ``rowwise_adagrad_row`` (the sorted
  route and the dense kernel; csrc/table_rules.h) on the VEC = ``vec`` path."""
  d = np.shape(g)[-1]
  assert vec in (1, 4) and d % vec == 0
  return _butterfly(_lane_partials(g, vec, group_lanes(d, vec)))


def sum_squares_rowscan_order(g):
  """The same sum in the row scan's order (``rowscan_rowwise``): lane l of the wave owns the features l, l + 64, l + 128,
  l + 192, ascending, then the butterfly over 64 lanes."""
  assert np.shape(g)[-1] <= 256
  return _butterfly(_lane_partials(g, 1, 64))


def rowwise_accumulators(rng, rows):
  """One accumulator per row in 0.5 .. 2 x 1e-6: BELOW a row's mean square gradient (about 9e-6), so the last bits of
  the sum of squares survive in acc' = acc + s.  (Under the suite's 0.025 .. 0.225 they are rounded away and any order
  of the sum gives the same accumulator.)"""
  return (rng.uniform(0.5, 2.0, size=rows) * 1e-6).astype(np.float32)


def rowwise_case(rows, d, seed=0):
  """Weights about 1e-3 N(0, 1), ``rowwise_accumulators``, gradients about 3e-3 N(0, 1) with every fifth row (4, 9,
  ...) all +0.  Returns (w, acc, g)."""
  rng = np.random.default_rng(80_000 + 1000 * seed + 7 * rows + d)
  w = rule_weights(rng, (rows, d))
  acc = rowwise_accumulators(rng, rows)
  g = (rng.normal(size=(rows, d)) * 3e-3).astype(np.float32)
  g[4::5] = 0.0
  return w, acc, g
