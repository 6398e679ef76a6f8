"""NumPy restatement of ``optimizers.SGD`` / ``Adam`` / ``Ftrl`` (recommenders_amd/optimizers.py; the ``update_step`` of
the Keras optimizers of the same names) in float64 and -- in the kernels' operation order -- in float32, and the derived
error bounds that the GPU kernels and the float32 restatement itself are held to against the float64 restatement on the
same float32 inputs.  Duplicates of a sparse gradient are summed in float32 in occurrence order in BOTH variants
(``clippy_restatement.sum_duplicates``: the project's contract for IndexedSlices), so the summed gradient is an input,
not an error source.  Test infrastructure only.

What the build guarantees (recommenders_amd/csrc/build.py: ``-O3 -std=c++17 -fPIC`` and nothing else for
sparse_update.hip and table_update.hip -- no fast-math flag, so hipcc's default ``-fhip-fp32-correctly-rounded-divide-sqrt`` holds):
division and ``sqrtf`` are correctly rounded.  hipcc contracts ``a * b + c`` by default; csrc/table_rules.h switches
contraction off inside every rule, so each operation rounds on its own as in NumPy.

Bounds.  u = 2^-24 (round to nearest); E_x is the first-order bound on the error of x, every final bound is
2 * (first-order bound): the factor 2 covers the second-order terms.  A hyper-parameter is a double in the float64
restatement and is rounded to float32 once in the kernels: one rounding each.  Values (m', D, ...) are the float64
restatement's.

  SGD   w' = w - lr g              lr, product, difference                           E_w = u (2 |lr g| + |w'|)

  Adam  alpha                      float64 from the integer t, rounded once; the float64 chain itself (<= 130
                                   products, a root, a quotient; the cancellation 1 - beta^t amplifies by at most
                                   1 / (1 - beta) = 1000) stays below 1e-10 relative      E_alpha = 1.001 u alpha
        m' = m + T1, T1 = (g - m) c1        c1, difference, product, sum              E_m = u (3 |T1| + |m'|)
        v' = v + T2, T2 = (g g - v) c2      g g (enters T2 as u g^2 c2), c2, difference, product, sum
                                                                                      E_v = u (3 |T2| + c2 g^2 + |v'|)
        w' = w - D, D = m' alpha / den, den = sqrt(v') + eps
              m' alpha: E_m alpha + 2 u |m' alpha| (alpha's own rounding, the product)
              den: sqrt carries E_v / (2 sqrt v') and its own rounding, eps its rounding, the sum its rounding:
                   E_den <= E_v / (2 sqrt v') + 2 u den
              quotient and difference: one rounding each
                                   E_w = E_m alpha / den + |D| (5 u + E_v / (2 sqrt(v') den)) + u |w'|

  Ftrl  n' = n + g g               product, sum                                      E_n = u (g^2 + n')
        g' = g + c w, c = 2 shrink          c, product, sum                          E_g' = u (2 |c w| + |g'|)
        P' = sqrt(n'), P = sqrt(n)          E_P' = E_n / (2 P') + u P',  E_P = u P   (power 0: P' = P = 1 exactly)
        S = (P' - P) / lr * w      THE DIFFERENCE CANCELS: its error is absolute in P', not relative to P' - P
                                   E_diff = E_P' + E_P + u |P' - P|;  / lr: lr's rounding and the quotient's;  * w
                                   E_S = (E_diff / lr + 2 u |P' - P| / lr) |w| + u |S|  ~  2.5 u sqrt(n') / lr |w|
        lin' = lin + (g' - S)      two sums                                          E_lin = E_g' + E_S + u |g' - S| + u |lin'|
        q = P' / lr + k, k = 2 l2r          lr, quotient, k, sum                     E_q = E_P' / lr + 2 u P' / lr + u k + u q
        N = clip(lin', -l1, l1) - lin'      l1's rounding where clipped, the difference (unclipped: exactly 0 on both
                                   sides; an element that only one side clips is within E_lin + u l1 of 0)
                                                                                      E_N = u l1 + E_lin + u |N|
        w' = N / q                                                                   E_w = E_N / q + |w'| E_q / q + u |w'|

The band checks bite only if a step moves ``w`` by much more than its bound: ``sparse_case`` divides the rows of the
cases without outliers by the largest duplicate count (> 1000), so a tail row's gradient is about 3e-3 / 1900 = 1.6e-6
and 5 % of the elements are below 0.063 of that.  Adam's step is of unit scale (about ``lr`` whatever |g|, down to
|g| ~ epsilon / sqrt(1 - beta_2)): 0.001 is enough.  SGD moves by ``lr |g|`` against a bound of about 2 u |w| <= 1.8e-7
and needs lr |g| > 1.8e-5 at |g| = 1e-7: ``SGD_LR = 256``.  Ftrl from a consistent state moves by ``lr |g| / sqrt(n')``,
sqrt(n') <= 0.48, against about 7 u |w| <= 6.3e-7: ``FTRL_LR = 512``.  (Powers of two: the float32 rate is the double.)
"""

import numpy as np

from tests import clippy_restatement as crs

U = 2.0 ** -24

SGD_LR = 256.0
FTRL_LR = 512.0
ADAM_LR = 0.001

# name -> (optimizer class name, keyword arguments); the slots of each rule in kernel order
RULES = {
    "sgd": ("SGD", dict(learning_rate=SGD_LR)),
    "adam": ("Adam", dict(learning_rate=ADAM_LR, beta_1=0.9, beta_2=0.999, epsilon=1e-7)),
    "ftrl": ("Ftrl", dict(learning_rate=FTRL_LR)),
    "ftrl_reg": ("Ftrl", dict(learning_rate=FTRL_LR, l1_regularization_strength=1e-5, l2_regularization_strength=1e-4,
                              l2_shrinkage_regularization_strength=1e-5, beta=0.05)),
    "ftrl_power0": ("Ftrl", dict(learning_rate=FTRL_LR, learning_rate_power=0.0, l2_regularization_strength=1e-5, beta=0.01)),
}
SLOTS = {"SGD": (), "Adam": ("m", "v"), "Ftrl": ("accumulator", "linear")}

_FTRL_DEFAULTS = dict(learning_rate=0.001, learning_rate_power=-0.5, initial_accumulator_value=0.1,
                      l1_regularization_strength=0.0, l2_regularization_strength=0.0,
                      l2_shrinkage_regularization_strength=0.0, beta=0.0)


def adam_alpha(hp, t):
  """float64 ``lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)`` for the integer ``t`` = iterations + 1."""
  return hp["learning_rate"] * np.sqrt(1.0 - hp["beta_2"] ** int(t)) / (1.0 - hp["beta_1"] ** int(t))


def initial_slots(kind, hp, w):
  if kind == "Adam":
    return [np.zeros_like(w), np.zeros_like(w)]
  if kind == "Ftrl":
    return [np.full_like(w, hp.get("initial_accumulator_value", 0.1)), np.zeros_like(w)]
  return []


def ftrl_consistent_linear(hp, w, n):
  """The ``linear`` slot a table at ``w`` with accumulator ``n`` would have without regularisers, -w n^p / lr (float32
  arithmetic: it is a starting state, not a result)."""
  hp = dict(_FTRL_DEFAULTS, **hp)
  lr = np.float32(hp["learning_rate"])
  return -w * np.sqrt(n) / lr if hp["learning_rate_power"] != 0.0 else -w / lr


def update(kind, w, slots, g, hp, dtype, alpha=None):
  """One step of rule ``kind`` on same-shaped ``w, slots, g`` in ``dtype`` arithmetic, in the kernels' operation order.
  ``alpha``: Adam's step size (float64 from ``adam_alpha``; the float32 variant rounds it once, as the device does).
  Returns a dict: w, slots (list) and the intermediates the bounds need."""
  t = np.dtype(dtype).type
  w, g = np.asarray(w, dtype=dtype), np.asarray(g, dtype=dtype)
  slots = [np.asarray(s, dtype=dtype) for s in slots]
  if kind == "SGD":
    step = t(hp["learning_rate"]) * g
    return dict(w=w - step, slots=[], step=step)
  if kind == "Adam":
    m, v = slots
    c1, c2, eps, a = t(1.0 - hp["beta_1"]), t(1.0 - hp["beta_2"]), t(hp["epsilon"]), t(alpha)
    t1 = (g - m) * c1
    m2 = m + t1
    t2 = (g * g - v) * c2
    v2 = v + t2
    den = np.sqrt(v2) + eps
    step = m2 * a / den
    return dict(w=w - step, slots=[m2, v2], t1=t1, t2=t2, den=den, step=step, alpha=a, c2=c2)
  if kind == "Ftrl":
    hp = dict(_FTRL_DEFAULTS, **hp)
    n, lin = slots
    lr, l1 = t(hp["learning_rate"]), t(hp["l1_regularization_strength"])
    k = t(2.0 * (hp["l2_regularization_strength"] + hp["beta"] / (2.0 * hp["learning_rate"])))
    c = t(2.0 * hp["l2_shrinkage_regularization_strength"])
    root = hp["learning_rate_power"] != 0.0
    gp = g + c * w
    n2 = n + g * g
    pn2 = np.sqrt(n2) if root else np.ones_like(n2)
    pn = np.sqrt(n) if root else np.ones_like(n)
    s = (pn2 - pn) / lr * w
    inner = gp - s
    lin2 = lin + inner
    q = pn2 / lr + k
    num = np.minimum(np.maximum(lin2, -l1), l1) - lin2
    return dict(w=num / q, slots=[n2, lin2], gp=gp, cw=c * w, pn2=pn2, pn=pn, s=s, inner=inner, q=q, num=num, k=k,
                l1=l1, lr=lr, root=root)
  raise ValueError(kind)


def piece_length(d):
  """Positions per piece of a long run on the sorted route (``tfrs_embedding_scatter_add_unsorted`` and
  ``tfrs_table_update_sparse``: the power of two >= max(32, d))."""
  piece = 32
  while piece < d:
    piece *= 2
  return piece


def sum_duplicates(ids, rows, vocab, piece=None):
  """(unique valid ids ascending, their float32 gradient rows summed in the order the route sums them).

  ``piece=None`` (the row scan): ``clippy_restatement.sum_duplicates``, one chain per id in occurrence order from +0.
  ``piece`` (the sorted route, ``piece_length(d)``): the order of the sparse Adagrad path (``scatter_add_u32_kernel`` with
  ``scatter_add_pieces_kernel``), whose bits ``SGD(lr=1)`` on a zero table is tested to equal.  In the stably sorted list
  of the valid ids a run that starts at position i is cut at the multiples of ``piece`` from
  ``(ceil(i / piece) + 1) * piece`` on; every piece is one occurrence-order chain from +0, and the pieces are then added
  to the first one in order.  A run that ends before its first cut -- every run shorter than ``piece`` -- is one chain
  as on the row scan.  The sums differ from the single chain only by float32 reassociation, but they ARE the rule's
  input: an error bound that counts the roundings of the rule alone has to be taken from them."""
  if piece is None:
    return crs.sum_duplicates(ids, rows, vocab)
  ids = np.asarray(ids).reshape(-1).astype(np.int64)
  rows = np.asarray(rows, dtype=np.float32).reshape(ids.size, -1)
  keep = (ids >= 0) & (ids < vocab)
  ids, rows = ids[keep], rows[keep]
  if not ids.size:
    return ids, rows
  order = np.argsort(ids, kind="stable")
  sorted_ids = ids[order]
  pos = np.arange(ids.size)
  is_start = np.r_[True, sorted_ids[1:] != sorted_ids[:-1]]
  run = np.cumsum(is_start) - 1
  start = pos[is_start][run]
  first_end = ((start + piece - 1) // piece + 1) * piece
  rank = np.where(pos < first_end, 0, (pos - first_end) // piece + 1)          # piece number inside the run
  is_piece_start = is_start | np.r_[False, rank[1:] != rank[:-1]]
  label = np.cumsum(is_piece_start) - 1
  original = np.empty_like(label)
  original[order] = label                                                      # piece of every occurrence, unsorted
  _, sums = crs.sum_duplicates(original, rows, int(label[-1]) + 1)             # each piece: one chain from +0
  piece_run, piece_rank = run[is_piece_start], rank[is_piece_start]
  g = sums[piece_rank == 0].copy()
  for r in range(1, int(piece_rank.max()) + 1):
    sel = piece_rank == r
    g[piece_run[sel]] += sums[sel]
  return sorted_ids[is_start], g


def sparse_update(kind, table, slots, ids, rows, hp, dtype, alpha=None):
  """The step on the touched rows only: dict as ``update`` over ``[len(uniq), d]`` plus ``uniq`` and ``g`` (the summed
  float32 gradient)."""
  uniq, g = crs.sum_duplicates(ids, rows, table.shape[0])
  out = update(kind, np.asarray(table)[uniq], [np.asarray(s)[uniq] for s in slots], g, hp, dtype, alpha)
  out.update(uniq=uniq, g=g)
  return out


def bounds(kind, ref64, g, w_before):
  """The module docstring's bounds from the float64 step ``ref64``: dict with ``w`` and one entry per slot."""
  g = np.asarray(g, dtype=np.float64)
  aw = np.abs(ref64["w"])
  if kind == "SGD":
    return dict(w=2 * U * (2 * np.abs(ref64["step"]) + aw))
  if kind == "Adam":
    m2, v2 = ref64["slots"]
    e_m = U * (3 * np.abs(ref64["t1"]) + np.abs(m2))
    e_v = U * (3 * np.abs(ref64["t2"]) + ref64["c2"] * g * g + np.abs(v2))
    root = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
      from_v = np.where(e_v > 0, e_v / (2 * root * ref64["den"]), 0.0)     # (v' = 0 only with g = 0 and v = 0: E_v = 0)
    e_w = e_m * ref64["alpha"] / ref64["den"] + np.abs(ref64["step"]) * (5 * U + from_v) + U * aw
    return dict(w=2 * e_w, m=2 * e_m, v=2 * e_v)
  if kind == "Ftrl":
    n2, lin2 = ref64["slots"]
    lr, q, pn2, pn = ref64["lr"], ref64["q"], ref64["pn2"], ref64["pn"]
    w0 = np.abs(np.asarray(w_before, dtype=np.float64))
    e_n = U * (g * g + n2)
    e_gp = U * (2 * np.abs(ref64["cw"]) + np.abs(ref64["gp"]))
    if ref64["root"]:
      e_pn2, e_pn = e_n / (2 * pn2) + U * pn2, U * pn
    else:
      e_pn2, e_pn = 0.0, 0.0
    diff = np.abs(pn2 - pn)
    e_s = ((e_pn2 + e_pn + U * diff) / lr + 2 * U * diff / lr) * w0 + U * np.abs(ref64["s"])
    e_lin = e_gp + e_s + U * np.abs(ref64["inner"]) + U * np.abs(lin2)
    e_q = e_pn2 / lr + 2 * U * pn2 / lr + U * ref64["k"] + U * q
    e_num = U * ref64["l1"] + e_lin + U * np.abs(ref64["num"])
    e_w = e_num / q + aw * e_q / q + U * aw
    return dict(w=2 * e_w, accumulator=2 * e_n, linear=2 * e_lin)
  raise ValueError(kind)


def check_step(kind, got_w, got_slots, w_before, ref64, g, label=""):
  """Asserts the bounds for one variable's step: ``got_*`` (float32 results) against ``ref64`` (``update(...,
  np.float64)`` from the same float32 state and gradient).  Returns the observed fraction of each budget."""
  b = bounds(kind, ref64, g, w_before)
  used = {}
  pairs = [("w", got_w, ref64["w"])] + [(key, got, ref) for key, got, ref in zip(SLOTS[kind], got_slots, ref64["slots"])]
  for key, got, ref in pairs:
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert err.shape == np.shape(b[key])
    used[key] = float((err / np.maximum(b[key], 1e-300)).max()) if err.size else 0.0
    assert (err <= b[key]).all(), f"{label} {key}: {used[key]:.3f} of the bound"
  return used


def moved_fraction(kind, ref64, g, w_before):
  """Fraction of the elements with a non-zero gradient whose float64 step moves ``w`` by more than 100 x its bound."""
  g = np.asarray(g)
  nonzero = g != 0
  if not nonzero.any():
    return 1.0
  moved = np.abs(ref64["w"] - np.asarray(w_before, dtype=np.float64)) > 100 * bounds(kind, ref64, g, w_before)["w"]
  return float(moved[nonzero].mean())


def check_alpha(got, hp, t):
  """Adam's device step size against the float64 formula: one rounding."""
  ref = adam_alpha(hp, t)
  assert abs(float(got) - ref) <= 1.001 * U * ref, (float(got), ref, t)
  return abs(float(got) - ref) / (1.001 * U * ref)


def dense_case(name, steps=2):
  """The randomized dense case of rule ``name``, the same in the CPU and the GPU tests: (sizes, weights per tensor,
  gradients per step and tensor); every second tensor carries outlier gradients."""
  rng = np.random.default_rng(500 + sorted(RULES).index(name))
  sizes = crs.dense_sizes(rng)
  ws = [crs.weights(rng, (n,)) for n in sizes]
  grads = [[crs.gradients(rng, (n,), outliers=(i % 2 == 0)) for i, n in enumerate(sizes)] for _ in range(steps)]
  return sizes, ws, grads


def sparse_rng(name, d):
  return np.random.default_rng(1000 * (10 + sorted(RULES).index(name)) + d)


def start_slots(name, table, acc):
  """Slots a sparse case starts from: Adam's own zeros; Ftrl at accumulator ``acc`` (0.025 .. 0.225, as ``sparse_case``
  draws it) with the linear slot of a table that Ftrl itself had brought to ``table``."""
  kind, hp = RULES[name]
  if kind == "Ftrl":
    return [acc.copy(), ftrl_consistent_linear(hp, table, acc)]
  return initial_slots(kind, hp, table)


_SPARSE_CACHE = {}


def sparse_cases(d):
  """The randomized sparse cases at feature width ``d``, the same for every rule and in the CPU and the GPU tests: one
  per ``clippy_restatement.SPARSE_SHAPES`` entry, each a dict with the table, ``acc`` (0.025 .. 0.225) and the
  ``(ids, rows)`` slices of two consecutive steps (Zipf ids with duplicates, negative, out-of-range and INT_MAX ids mixed
  in; step one has a touched row whose summed gradient is exactly zero).  Computed once per ``d`` (the last one is kept)
  and read-only."""
  if d not in _SPARSE_CACHE:
    _SPARSE_CACHE.clear()
    rng = np.random.default_rng(7000 + d)
    cases = []
    for vocab, n, outliers, id_dtype in crs.SPARSE_SHAPES:
      table, acc, ids, rows = crs.sparse_case(rng, vocab, n, d, outliers, id_dtype)
      ids2 = crs.zipf_ids(rng, n, vocab)
      ids2[::89] = -5
      ids2[3::107] = vocab
      ids2[11::109] = np.iinfo(id_dtype).max
      rows2 = crs.gradients(rng, (n, d), outliers)
      if not outliers:
        rows2 /= np.float32(np.bincount(ids2[(ids2 >= 0) & (ids2 < vocab)]).max())
      steps = [(ids, rows), (ids2.astype(id_dtype), rows2)]
      for a in (table, acc, ids, rows, steps[1][0], rows2):
        a.setflags(write=False)
      cases.append(dict(vocab=vocab, n=n, outliers=outliers, table=table, acc=acc, steps=steps))
    _SPARSE_CACHE[d] = cases
  return _SPARSE_CACHE[d]
