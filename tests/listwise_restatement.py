"""Float64 restatement of the listwise ranking losses and of NDCG, written from the formulas with
explicit loops over pairs and ranks, plus the error bounds the GPU tests hold the kernels to.  Test infrastructure
only: it shares no code with the product.

Formulas (one list; y labels, s scores, V = {i : y_i >= 0}, n = |V|):
  softmax            l = sum_{i in V} y_i (lse - s_i),  lse = m + log sum_V exp(s_i - m),  m = max_V s
                     dl/ds_k = (sum_V y) exp(s_k - lse) - y_k
  pairwise           P = {(i, j) in V^2 : y_i > y_j},  l = sum_P phi(s_i - s_j)
    logistic         phi(x) = max(-x, 0) + log1p(exp(-|x|)),  phi'(x) = -1 / (1 + exp(x))
    hinge            phi(x) = max(0, 1 - x),  phi'(x) = -1 for x < 1 else 0
                     dl/ds_k = sum_{(k, j) in P} phi'(s_k - s_j) - sum_{(i, k) in P} phi'(s_i - s_k)
  ListMLE            pi = V by label descending, ties by position ascending;  lse_r = logsumexp_{t >= r} s_pi(t)
                     l = sum_{r < n} (lse_r - s_pi(r)),  dl/ds_pi(t) = -1 + sum_{r <= t} exp(s_pi(t) - lse_r)
  NDCG               sigma = V by score descending, ties by position ascending;
                     DCG = sum_{r < min(n, topn)} (2^{y_sigma(r)} - 1) / log2(r + 2),  IDCG the same in pi order;
                     a list counts iff IDCG > 0;  result = sum_b w_b DCG_b / IDCG_b / sum_b w_b over the counted lists.

The bound.  eps = 2^-24 is the unit roundoff of float32.  An output that is a sum of n terms, each computed with a
relative error of at most u eps, is within
    (n - 1 + u) * eps * sum |terms|
of the exact value for ANY summation order (n - 1 additions, each rounding a partial sum that is at most sum |terms|,
to first order), so no test built on it pins an order.  Every entry below therefore comes with its number of addends
``n``, its yardstick ``yard`` and its ``u``; ``bound(n, yard, u)`` is the line above and ``gate_yardstick`` puts it
into the form tests/conftest.py: float_gate takes (limit eps).

u counts the library calls and roundings that make a term.  ROCm's published ulp table for the device math functions
is not part of this tree, so every call of expf, logf, log1pf, exp2f, log2f and every division is charged 4 ulp
(= 4 eps); an addition, subtraction or multiplication is charged 1.  A term that goes through exp of a ROUNDED argument a inherits the argument's ABSOLUTE
error as its relative error, so such a term enters the yardstick multiplied by its condition (1 + |a| and the like):
  pairwise logistic  x = s_i - s_j carries eps |x|; exp(-|x|) then (4 + |x|) eps; log1p of it 4 more (its condition is
                     <= 1), the max(-x, 0) part 1, the addition 1:  u = 10, the term's yardstick phi(x) (1 + |x|).  phi'
                     likewise (exp, 1 + e, a division): u = 10, yardstick |phi'(x)| (1 + |x|).
  pairwise hinge     1 - x after x = s_i - s_j: absolute error eps (|x| + |1 - x|) <= 2 eps (1 + |x|): u = 2, yardstick
                     1 + |x| for an active pair (and for a pair within 1e-6 of the kink, which may round to either
                     side); phi' is exact.
  logsumexp          S = sum_V exp(s_i - m) lies in [1, n]; its terms carry <= 6 eps of S each and k of them are summed
                     (in any order, possibly through a scan of (max, sum) pairs, whose rescalings add <= 7 eps per
                     level and at most 10 levels): S has relative error <= (k + 80) eps, log S the same as an absolute
                     error plus 4 eps |log S|, the final m + log S one rounding:
                         |lse~ - lse| <= (k + 85) eps T,   T = 1 + |m| + |log S|.
  softmax            term y_i (lse - s_i): u = n + 87, yardstick y_i (T + |lse - s_i|).  Gradient: (sum_V y) has n - 1
                     roundings, exp(s_k - lse) inherits the absolute error of its argument: u = 2 n + 95, yardstick
                     (sum y) exp(s_k - lse) (T + |s_k - lse|), plus the exact addend y_k.
  ListMLE            term lse_r - s_pi(r): u = n + 87, yardstick T_r + |lse_r - s_pi(r)|.  Gradient: G = sum_{r <= t}
                     exp(s_pi(t) - lse_r) may be formed as exp(s_pi(t) + logsumexp_{r <= t}(-lse_r)): the inner
                     logsumexp adds (n + 85) eps max_r T_r of its inputs' errors to its own (n + 85) eps (1 + |q|):
                     u = 2 n + 180, yardstick G (1 + max_r T_r + |log G|), plus the exact addend 1; counted as t + 2
                     addends so that a direct sum over r is covered too.
  NDCG               a term (2^y - 1) / log2(r + 2): exp2f, a subtraction that cancels for small y (so the yardstick is
                     2^y / log2(r + 2), not the term), log2f of an exact integer, a division: u = 13.  The ratio:
                     |ndcg~ - ndcg| <= b_DCG / IDCG + ndcg (b_IDCG / IDCG + eps)   (the two relative bounds + one
                     rounding).
Absolute floor: a float32 result below the smallest normal number (2^-126) may be flushed to zero, so every gate
built from these bounds allows an absolute 2^-126 (float_gate(..., floor=FLOOR / EPS)).
"""

import math

import numpy as np

EPS = 2.0 ** -24
FLOOR = 2.0 ** -126
SOFTMAX, PAIRWISE_LOGISTIC, PAIRWISE_HINGE, LIST_MLE = 0, 1, 2, 3
KINDS = {"softmax": SOFTMAX, "pairwise_logistic": PAIRWISE_LOGISTIC, "pairwise_hinge": PAIRWISE_HINGE,
         "list_mle": LIST_MLE}
MAX_LIST_LEN = 1024


def bound(n, yard, u):
  return (np.maximum(np.asarray(n, dtype=np.float64) - 1.0, 0.0) + u) * EPS * np.asarray(yard, dtype=np.float64)


def gate_yardstick(n, yard, u):
  """float_gate(got, ref, gate_yardstick(...), limit=EPS, floor=FLOOR / EPS) asserts |got - ref| <= max(bound(n, yard, u),
  FLOOR): float_gate floors the yardstick, so the floor is passed in the yardstick's unit."""
  return bound(n, yard, u) / EPS


class Entry:
  """value, addends, yardstick and u of one output entry (or of an array of them)."""

  def __init__(self, value, n, yard, u):
    self.value, self.n, self.yard, self.u = value, n, yard, u

  @property
  def bound(self):
    return bound(self.n, self.yard, self.u)

  @property
  def gate(self):
    return gate_yardstick(self.n, self.yard, self.u)


def _valid(y):
  return [i for i in range(len(y)) if y[i] >= 0.0]


def _logsumexp(vals):
  """(lse, m, log S) of a non-empty list."""
  m = max(vals)
  logs = math.log(sum(math.exp(v - m) for v in vals))
  return m + logs, m, logs


def _phi(kind, x):
  if kind == PAIRWISE_HINGE:
    return max(0.0, 1.0 - x)
  return max(-x, 0.0) + math.log1p(math.exp(-abs(x)))


def _dphi(kind, x):
  if kind == PAIRWISE_HINGE:
    return -1.0 if x < 1.0 else 0.0
  e = math.exp(-abs(x))
  return -e / (1.0 + e) if x >= 0.0 else -1.0 / (1.0 + e)


def _pair_yard(kind, x, val):
  if kind == PAIRWISE_HINGE:
    return (1.0 + abs(x)) if x < 1.0 + 1e-6 else 0.0
  return abs(val) * (1.0 + abs(x))


def label_order(y):
  """pi: valid positions by label descending, ties by position ascending."""
  return sorted(_valid(y), key=lambda i: (-y[i], i))


def score_order(y, s):
  """sigma: valid positions by score descending, ties by position ascending."""
  return sorted(_valid(y), key=lambda i: (-(s[i] + 0.0), i))


def list_loss(kind, y, s):
  """One list: (Entry of the loss, Entry of the gradient [L]).  y, s: sequences of floats (used as float64)."""
  y = [float(v) for v in y]
  s = [float(v) for v in s]
  L = len(y)
  V = _valid(y)
  n = len(V)
  g = np.zeros(L)
  gn = np.zeros(L)
  gy = np.zeros(L)
  if kind == SOFTMAX:
    if n == 0:
      return Entry(0.0, 0, 0.0, 0.0), Entry(g, gn, gy, 0.0)
    lse, m, logs = _logsumexp([s[i] for i in V])
    T = 1.0 + abs(m) + abs(logs)
    ysum = sum(y[i] for i in V)
    val = yard = 0.0
    for i in V:
      val += y[i] * (lse - s[i])
      yard += y[i] * (T + abs(lse - s[i]))
    for k in V:
      p = ysum * math.exp(s[k] - lse)
      g[k] = p - y[k]
      gn[k] = 2
      gy[k] = p * (T + abs(s[k] - lse)) + y[k]
    return Entry(val, n, yard, n + 87.0), Entry(g, gn, gy, 2.0 * n + 95.0)
  if kind in (PAIRWISE_LOGISTIC, PAIRWISE_HINGE):
    val = yard = 0.0
    cnt = 0
    for i in V:
      for j in V:
        if y[i] > y[j]:
          x = s[i] - s[j]
          v = _phi(kind, x)
          d = _dphi(kind, x)
          val += v
          yard += _pair_yard(kind, x, v)
          cnt += 1
          g[i] += d
          g[j] -= d
          gn[i] += 1
          gn[j] += 1
          dy = abs(d) * (1.0 + abs(x)) if kind == PAIRWISE_LOGISTIC else abs(d)
          gy[i] += dy
          gy[j] += dy
    u = 2.0 if kind == PAIRWISE_HINGE else 10.0
    return Entry(val, cnt, yard, u), Entry(g, gn, gy, u if kind == PAIRWISE_LOGISTIC else 0.0)
  if kind == LIST_MLE:
    pi = label_order(y)
    val = yard = 0.0
    lses = []
    Ts = []
    for r in range(n):
      lse, m, logs = _logsumexp([s[pi[t]] for t in range(r, n)])
      lses.append(lse)
      Ts.append(1.0 + abs(m) + abs(logs))
      val += lse - s[pi[r]]
      yard += Ts[r] + abs(lse - s[pi[r]])
    for t in range(n):
      G = 0.0
      for r in range(t + 1):
        G += math.exp(s[pi[t]] - lses[r])
      g[pi[t]] = -1.0 + G
      gn[pi[t]] = t + 2
      gy[pi[t]] = G * (1.0 + max(Ts[:t + 1]) + abs(math.log(G))) + 1.0
    return Entry(val, n, yard, n + 87.0), Entry(g, gn, gy, 2.0 * n + 180.0)
  raise ValueError(kind)


def batch_loss(kind, y, s):
  """[B, L] arrays -> (Entry of the per-list losses [B], Entry of the gradients [B, L]) of the UNWEIGHTED losses."""
  y = np.asarray(y, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  B, L = y.shape
  lv, ln, ly = np.zeros(B), np.zeros(B), np.zeros(B)
  gv, gn, gy = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
  lu = gu = 0.0
  for b in range(B):
    le, ge = list_loss(kind, y[b], s[b])
    lv[b], ln[b], ly[b] = le.value, le.n, le.yard
    gv[b], gn[b], gy[b] = ge.value, ge.n, ge.yard
    lu, gu = max(lu, le.u), max(gu, ge.u)
  return Entry(lv, ln, ly, lu), Entry(gv, gn, gy, gu)


def _dcg(order, y, topn):
  val = yard = 0.0
  cnt = 0
  lim = len(order) if topn is None else min(len(order), topn)
  for r in range(lim):
    disc = math.log2(r + 2.0)
    val += (2.0 ** y[order[r]] - 1.0) / disc
    yard += 2.0 ** y[order[r]] / disc
    cnt += 1
  return Entry(val, cnt, yard, 13.0)


def list_ndcg(y, s, topn=None):
  """One list: (ndcg, counted, bound on |ndcg~ - ndcg|)."""
  y = [float(v) for v in y]
  s = [float(v) for v in s]
  dcg = _dcg(score_order(y, s), y, topn)
  idcg = _dcg(label_order(y), y, topn)
  if not idcg.value > 0.0:
    return 0.0, 0.0, 0.0
  v = dcg.value / idcg.value
  return v, 1.0, float(dcg.bound / idcg.value + v * (idcg.bound / idcg.value + EPS))


def batch_ndcg(y, s, topn=None):
  rows = [list_ndcg(y[b], s[b], topn) for b in range(len(y))]
  return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


def ndcg_result(batches, topn=None):
  """Metric result over several (y, s, w or None) updates: (value, bound).  The weighted mean adds, to the per-list
  bounds, one rounding per product and per addition of the two sums and the final division: (2 B + 4) eps of the
  result (B = all lists seen)."""
  tot = cnt = bnd = 0.0
  nb = 0
  for y, s, w in batches:
    v, c, e = batch_ndcg(y, s, topn)
    w = np.ones(len(v)) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    tot += float(np.sum(w * c * v))
    cnt += float(np.sum(w * c))
    bnd += float(np.sum(np.abs(w) * c * e))
    nb += len(v)
  if not cnt > 0.0:
    return 0.0, 0.0
  return tot / cnt, bnd / cnt + (2.0 * nb + 4.0) * EPS * abs(tot / cnt)


# ---- inputs shared by the host and the GPU tests ---------------------------------------------------------------------
# B in {1, 3, 67} x L: the lengths on both sides of every switch of the work mapping (a group of 8 / 16 / 32 / 64
# lanes per list, then a 256-thread workgroup with 1 .. 4 items per thread) and the top of the envelope.
LENGTHS = (1, 2, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 256, 257, 1024)
SHAPES = tuple((b, l) for l in LENGTHS for b in ((3,) if l == 1024 else (1, 3, 67)))


def make_labels(B, L, seed):
  """Labels in {-1, 0, 1, 2, 3, 4}: padding in the middle (about one position in six) and a padded tail of varying
  length (list 0 keeps every tail position)."""
  rng = np.random.RandomState(seed)
  y = rng.randint(-1, 5, size=(B, L)).astype(np.float32)
  for b in range(1, B):
    tail = rng.randint(0, max(L // 3, 1) + 1)
    if tail:
      y[b, L - tail:] = -1.0
  return y


def make_scores(B, L, seed, std=2.0):
  return (np.random.RandomState(seed + 1).randn(B, L) * std).astype(np.float32)


def make_grid_scores(B, L, seed, step=0.25, lim=2.0):
  """Multiples of `step` in [-lim, lim]: few distinct values, so ties are planted by construction."""
  k = int(round(lim / step))
  return (np.random.RandomState(seed + 2).randint(-k, k + 1, size=(B, L)) * step).astype(np.float32)


def make_pow2_weights(B, seed):
  return (2.0 ** np.random.RandomState(seed + 3).randint(-1, 2, size=B)).astype(np.float32)


HINGE_STEP = 0.25


def hinge_exact_steps(y, s, w):
  """The exactness condition of the hinge test for one input set (scores on the HINGE_STEP grid, power-of-two
  weights, reduction "sum"): returns (ok, steps).  Every loss term max(0, 1 - x) is a non-negative integer multiple
  of q = HINGE_STEP, and so is every weighted term in units of q * min(w); because no term is negative, EVERY partial
  sum of ANY subset in ANY order lies between 0 and the total.  So if the total, in units of q * min(w), is an integer
  below 2^24, every intermediate of every summation order is an exactly representable float32 and the float32 result
  equals the exact one bit for bit.  Gradient entries are sums of +-1 (at most 2 L of them, every partial sum an
  integer of magnitude <= 2 L < 2^24) times a power of two: always exact."""
  y = np.asarray(y, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  w = np.asarray(w, dtype=np.float64)
  unit = HINGE_STEP * float(np.min(w))
  total = 0
  for b in range(y.shape[0]):
    V = _valid(y[b])
    for i in V:
      for j in V:
        if y[b, i] > y[b, j]:
          t = max(0.0, 1.0 - (s[b, i] - s[b, j])) * w[b] / unit
          if t != int(t):
            return False, -1
          total += int(t)
  return total < 2 ** 24 and 2 * y.shape[1] < 2 ** 24, total


def hinge_inputs(B, L):
  seed = 7000 + 13 * L + B
  return make_labels(B, L, seed), make_grid_scores(B, L, seed), make_pow2_weights(B, seed)
