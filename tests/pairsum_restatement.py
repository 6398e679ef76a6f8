"""Float64 restatement of the pair-sum losses (ApproxNDCG, ApproxMRR, UniqueSoftmax) and of their
gradients, written from the formulas with numpy row operations over one list at a time, plus the error bounds the GPU
tests hold the kernels to.  Test infrastructure only: it shares no code with the product.

Formulas (one list; y labels, s scores, V = {i : y_i >= 0}, n = |V|, alpha = float32(1 / temperature),
sigma(x) = 1 / (1 + e^-x), sigma'(x) = sigma(x) sigma(-x), G_i = 2^{y_i} - 1):
  soft rank      r_i = 1 + sum_{j in V, j != i} sigma(alpha (s_j - s_i))
  ApproxNDCG     l = -(1 / IDCG) sum_V G_i / log2(1 + r_i),  IDCG the ideal DCG of listwise_restatement over all n ranks
                 c_i = G_i / (IDCG ln2 (1 + r_i) log2(1 + r_i)^2)
  ApproxMRR      l = -(1 / Y) sum_V y_i / r_i,  Y = sum_V y_i;  c_i = y_i / (Y r_i^2)
                 both: dl/ds_k = alpha sum_{j in V, j != k} (c_j - c_k) sigma'(alpha (s_k - s_j));  l = 0 and every
                 gradient 0 where IDCG <= 0 (Y <= 0)
  UniqueSoftmax  t = alpha s,  lse_i = log(e^{t_i} + sum_{j in V: y_j < y_i} e^{t_j}),  l = sum_V G_i (lse_i - t_i)
                 dl/ds_k = alpha [G_k (e^{t_k - lse_k} - 1) + sum_{j in V: y_j > y_k} G_j e^{t_k - lse_j}]

The bounds follow the rules at the head of tests/listwise_restatement.py: eps = 2^-24; expf, logf, log2f, exp2f and a
division are charged 4 eps each, an addition, subtraction or multiplication 1 eps; a sum of n terms adds
(n - 1) eps sum |terms| in ANY order; an exp of a rounded argument carries the argument's absolute error as its
relative error; everything to first order in eps; the gates allow an absolute 2^-126.  Every bound below is an
ABSOLUTE bound b derived from the formulas; an Entry carries it as yard = b / ((n - 1 + u) eps), n the addends of the
outermost sum and u the largest per-term charge, so that Entry.bound == b.

  sigma          x = alpha (s_j - s_i): a subtraction and a product, |x~ - x| <= 2 eps |x|.  sigma from e = exp(-|x|),
                 d = 1 + e and one division: d log sigma / dx = 1 - sigma <= 1 gives 2 |x| eps, the exp 4, the addition 1,
                 the division 4: relative error (9 + 2 |x|) eps <= 10 eps (1 + |x|).
  soft rank      n addends (the leading 1 is exact): |r~_i - r_i| <= dr_i = (n - 1 + 10) eps R_i,
                 R_i = 1 + sum_j sigma_ij (1 + |x_ij|).
  sigma'         e / (d d): d log sigma' / dx = 1 - 2 sigma, at most 1 in size: 2 |x| eps; the exp 4, d twice 2, the
                 product 1, the division 4: (11 + 2 |x|) eps <= 11 eps (1 + |x|).
  IDCG           listwise_restatement._dcg: b_I = (n - 1 + 13) eps sum 2^y / log2(rank + 2).
  ApproxNDCG     term G_i / lg_i, lg_i = log2(1 + r_i) >= 1: G_i = exp2f - 1 is off by 5 eps 2^{y_i}; 1 + r_i by
                 eps (1 + r_i) + dr_i, which log2 turns into eps / ln2 + kappa_i dr_i relative to lg_i
                 (kappa_i = 1 / ((1 + r_i) ln2 lg_i)), log2f adds 4: lg_i has relative error 5.5 eps + kappa_i dr_i; the
                 division 4.  So a term is within 15 eps 2^{y_i} / lg_i + (G_i / lg_i) kappa_i dr_i, and the sum S within
                     b_S = (n - 1 + 15) eps sum_i (2^{y_i} / lg_i) (1 + kappa_i R_i)         (G <= 2^y, n + 9 <= n + 14).
                 l = -(S / IDCG), one division: b_l = b_S / IDCG + |l| (b_I / IDCG + 4 eps).
                 c_i: the constant ln2 1, 1 + r_i as above, lg_i twice (11 eps + 2 kappa_i dr_i), four products and one
                 division (8), IDCG b_I / IDCG, G_i 5 eps 2^{y_i}:
                     dc_i = 5 eps cbar_i + c_i (b_I / IDCG + 21 eps + dr_i (1 / (1 + r_i) + 2 kappa_i)),
                 cbar_i = c_i with 2^{y_i} for G_i.
  ApproxMRR      term y_i / r_i: within (y_i / r_i) (4 eps + dr_i / r_i); summed ((n - 1) eps), divided by Y (4 eps), which
                 itself is a sum of n labels ((n - 1) eps):
                     b_l = sum_i (y_i / (Y r_i)) ((2 n + 6) eps + dr_i / r_i).
                 c_i = y_i / ((Y r_i) r_i): two products, a division, Y, r_i twice:
                     dc_i = c_i ((n + 5) eps + 2 dr_i / r_i).
  approx gradient  term (c_j - c_k) sigma'_kj: the difference is off by dc_j + dc_k + eps |c_j - c_k|, sigma' as above, the
                 product 1; at most n - 1 terms are summed and the sum multiplied by alpha (1):
                     b_g_k = alpha [sum_j sigma'_kj (13 eps (1 + |x_kj|) |c_j - c_k| + dc_j + dc_k)
                                    + n eps sum_j |c_j - c_k| sigma'_kj].
  UniqueSoftmax  t_i = alpha s_i is off by eps |t_i|.  With M_i = {i} + {j : y_j < y_i}, k_i = |M_i|,
                 tau_i = max_{M_i} |t_j|, m_i = max_{M_i} t_j (a selection: exact) and a_i = sum_{M_i} exp(t_j - m_i) in
                 [1, n]: the rounded t move lse_i by at most eps tau_i; t_j - m_i is rounded once (<= 2 eps tau_i), so an
                 exp term has relative error (4 + 2 tau_i) eps and a_i (k_i - 1 + 4 + 2 tau_i) eps; logf adds
                 4 eps |log a_i|, the final addition eps |lse_i|:
                     dlse_i = eps (k_i + 3 + 3 tau_i + 4 |log a_i| + |lse_i|).
                 term G_i (lse_i - t_i), D_i = |lse_i - t_i|: G_i 5 eps 2^{y_i}, the difference dlse_i + eps |t_i| +
                 eps D_i, the product 1:
                     b_l = sum_i 2^{y_i} (7 eps D_i + dlse_i + eps |t_i|) + (n - 1) eps sum_i G_i D_i.
                 gradient: p_kj = exp(t_k - lse_j) <= 1 has the argument error A_kj = eps |t_k| + dlse_j +
                 eps |t_k - lse_j|, so a term G_j p_kj is within 2^{y_j} p_kj (10 eps + A_kj) (G 5, exp 4, product 1) and
                 the own term G_k (p_kk - 1) within 2^{y_k} (p_kk (4 eps + A_kk) + 7 eps) (the subtraction, G and the
                 product act on |p_kk - 1| <= 1); at most n terms, then alpha:
                     b_g_k = alpha [those + n eps (G_k |p_kk - 1| + sum_j G_j p_kj)].
"""

import math

import numpy as np

from tests.listwise_restatement import (EPS, FLOOR, SHAPES, Entry, bound, label_order, make_grid_scores,  # noqa: F401
                                        make_labels, make_pow2_weights, make_scores, _dcg)

APPROX_NDCG, APPROX_MRR, UNIQUE_SOFTMAX = 0, 1, 2
KINDS = {"approx_ndcg": APPROX_NDCG, "approx_mrr": APPROX_MRR, "unique_softmax": UNIQUE_SOFTMAX}
DEFAULT_TEMPERATURE = {"approx_ndcg": 0.1, "approx_mrr": 0.1, "unique_softmax": 1.0}
LN2 = math.log(2.0)


def alpha_of(temperature):
  """float32(1 / temperature) of the float32 temperature, as the C entry forms it."""
  return float(np.float32(1.0) / np.float32(temperature))


def entry_from_bound(value, n, u, b):
  """The Entry whose bound is the derived absolute bound b (see the module docstring)."""
  scale = (np.maximum(np.asarray(n, dtype=np.float64) - 1.0, 0.0) + u) * EPS
  return Entry(value, n, np.asarray(b, dtype=np.float64) / scale, u)


def scaled(entry, w, extra):
  """entry times the exact factor w, with `extra` more roundings of the result."""
  w = np.asarray(w, dtype=np.float64)
  v = entry.value * w
  return entry_from_bound(v, entry.n, entry.u, entry.bound * np.abs(w) + extra * EPS * np.abs(v))


def soft_ranks(sv, alpha):
  """(r, R, X, dsig) of the valid scores sv: X[i, j] = alpha (s_j - s_i), dsig = sigma'(X) with a zero diagonal."""
  n = len(sv)
  X = alpha * (sv[None, :] - sv[:, None])
  E = np.exp(-np.abs(X))
  sig = np.where(X >= 0.0, 1.0, E) / (1.0 + E)
  off = 1.0 - np.eye(n)
  r = 1.0 + (sig * off).sum(axis=1)
  R = 1.0 + (sig * off * (1.0 + np.abs(X))).sum(axis=1)
  return r, R, X, E / (1.0 + E) ** 2 * off


def list_loss(kind, y, s, temperature):
  """One list: (Entry of the loss, Entry of the gradient [L])."""
  y = np.asarray(y, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  alpha = alpha_of(temperature)
  L = len(y)
  V = np.nonzero(y >= 0.0)[0]
  n = len(V)
  g, gb = np.zeros(L), np.zeros(L)
  gn = np.zeros(L)
  gn[V] = n
  zero = (entry_from_bound(0.0, n, 1.0, 0.0), entry_from_bound(g, gn, 1.0, gb))
  if n == 0:
    return zero
  yv, sv = y[V], s[V]
  if kind == UNIQUE_SOFTMAX:
    t = alpha * sv
    own = np.eye(n, dtype=bool)
    M = (yv[None, :] < yv[:, None]) | own                     # M[i, j]: j enters lse_i
    m = np.where(M, t[None, :], -np.inf).max(axis=1)
    a = np.where(M, np.exp(np.minimum(t[None, :] - m[:, None], 0.0)), 0.0).sum(axis=1)
    lse = m + np.log(a)
    tau = np.where(M, np.abs(t)[None, :], 0.0).max(axis=1)
    dlse = EPS * (M.sum(axis=1) + 3.0 + 3.0 * tau + 4.0 * np.abs(np.log(a)) + np.abs(lse))
    G2 = 2.0 ** yv
    G = G2 - 1.0
    D = np.abs(lse - t)
    val = float(np.sum(G * (lse - t)))
    bl = float(np.sum(G2 * (7.0 * EPS * D + dlse + EPS * np.abs(t))) + (n - 1) * EPS * np.sum(G * D))
    U = (yv[None, :] > yv[:, None]) | own                     # U[k, j]: j enters g_k
    arg = t[:, None] - lse[None, :]
    Pm = np.where(U, np.exp(np.minimum(arg, 0.0)), 0.0)
    A = EPS * np.abs(t)[:, None] + dlse[None, :] + EPS * np.abs(arg)
    terms = np.where(own, G[None, :] * (Pm - 1.0), G[None, :] * Pm)
    err = np.where(own, G2[None, :] * (Pm * (4.0 * EPS + A) + 7.0 * EPS), G2[None, :] * Pm * (10.0 * EPS + A))
    g[V] = alpha * terms.sum(axis=1)
    gb[V] = alpha * (np.where(U, err, 0.0).sum(axis=1) + n * EPS * np.abs(terms).sum(axis=1))
    return entry_from_bound(val, n, 7.0, bl), entry_from_bound(g, gn, 10.0, gb)
  r, R, X, dsig = soft_ranks(sv, alpha)
  dr = (n - 1 + 10.0) * EPS * R
  if kind == APPROX_NDCG:
    ideal = _dcg(label_order(list(y)), list(y), None)
    I, bI = ideal.value, float(ideal.bound)
    if not I > 0.0:
      return zero
    G2 = 2.0 ** yv
    G = G2 - 1.0
    lg = np.log2(1.0 + r)
    kappa = 1.0 / ((1.0 + r) * LN2 * lg)
    val = -float(np.sum(G / lg)) / I
    bS = (n - 1 + 15.0) * EPS * float(np.sum(G2 / lg * (1.0 + kappa * R)))
    bl = bS / I + abs(val) * (bI / I + 4.0 * EPS)
    den = I * LN2 * (1.0 + r) * lg * lg
    c = G / den
    dc = 5.0 * EPS * G2 / den + c * (bI / I + 21.0 * EPS + dr * (1.0 / (1.0 + r) + 2.0 * kappa))
    ul = 15.0
  elif kind == APPROX_MRR:
    Y = float(np.sum(yv))
    if not Y > 0.0:
      return zero
    val = -float(np.sum(yv / r)) / Y
    bl = float(np.sum(yv / (Y * r) * ((2.0 * n + 6.0) * EPS + dr / r)))
    c = yv / (Y * r * r)
    dc = c * ((n + 5.0) * EPS + 2.0 * dr / r)
    ul = 4.0
  else:
    raise ValueError(kind)
  Cd = c[None, :] - c[:, None]                                # Cd[k, j] = c_j - c_k
  g[V] = alpha * (Cd * dsig).sum(axis=1)
  gb[V] = alpha * ((dsig * (13.0 * EPS * (1.0 + np.abs(X)) * np.abs(Cd) + dc[None, :] + dc[:, None])).sum(axis=1)
                   + n * EPS * (np.abs(Cd) * dsig).sum(axis=1))
  return entry_from_bound(val, n, ul, bl), entry_from_bound(g, gn, 13.0, gb)


def batch_loss(kind, y, s, temperature):
  """[B, L] arrays -> (Entry of the per-list losses [B], Entry of the gradients [B, L]) of the UNWEIGHTED losses."""
  y = np.asarray(y, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  B, L = y.shape
  lv, lb, ln = np.zeros(B), np.zeros(B), np.zeros(B)
  gv, gb, gn = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
  for b in range(B):
    le, ge = list_loss(kind, y[b], s[b], temperature)
    lv[b], lb[b], ln[b] = le.value, le.bound, le.n
    gv[b], gb[b], gn[b] = ge.value, ge.bound, ge.n
  return entry_from_bound(lv, ln, 1.0, lb), entry_from_bound(gv, gn, 1.0, gb)


# ---- the exact inputs of the ApproxMRR bit-for-bit test --------------------------------------------------------------
MRR_EXACT_N = (1, 3, 7, 15, 63, 127, 255, 1023)
MRR_EXACT_TEMPERATURES = (0.5, 0.125)


def mrr_exact_inputs(n):
  """Four lists of n valid items and one pad each (L = n + 1; the pad at the end, at the start, in the middle, at the
  end), all valid scores of a list equal, labels in {0, 1} with one or two ones, a poisoned pad score, power-of-two
  list weights."""
  L = n + 1
  y = np.zeros((4, L), dtype=np.float32)
  s = np.empty((4, L), dtype=np.float32)
  pads = (L - 1, 0, L // 2, L - 1)
  for b, (pad, level) in enumerate(zip(pads, (0.75, -1.5, 0.0, 3.0))):
    s[b] = level
    y[b, pad] = -1.0
    s[b, pad] = 1e30
    valid = [i for i in range(L) if i != pad]
    y[b, valid[0 if b % 2 == 0 else -1]] = 1.0
    if b >= 2 and n >= 2:
      y[b, valid[n // 2]] = 1.0
  w = np.array([1.0, 0.5, 2.0, 4.0], dtype=np.float32)
  return y, s, w


def _exact_sum(terms):
  """True iff every partial sum of every order of `terms` is a float32: with q the largest power of two that divides
  every term, sum |terms| / q < 2^24 (then every partial sum of every subset is an integer multiple of q below 2^24 q
  in size), and q and 2^24 q lie in the normal range."""
  terms = [abs(float(v)) for v in terms if v != 0.0]
  if not terms:
    return True

  def lowbit(v):      # the lowest set bit of the float64 v
    m, e = math.frexp(v)
    k = int(m * 2 ** 53)
    return 2.0 ** (e - 53 + (k & -k).bit_length() - 1)

  q = min(lowbit(v) for v in terms)
  if q < 2.0 ** -126 or any(v != float(np.float32(v)) for v in terms):
    return False
  return sum(int(v / q) for v in terms) < 2 ** 24 and sum(terms) < 2.0 ** 127


def mrr_exact_ok(y, s, w, temperature):
  """The exactness condition of the ApproxMRR bit-for-bit test: with all valid scores of a list equal every pair has
  x = 0 exactly, e = exp(0) = 1, sigma = 1 / 2 and sigma' = 1 / 4 exactly; what remains are sums, products and
  quotients, and each is checked to be exact in float32 in every order: the terms of r_i (1 and n - 1 halves), of Y,
  of the loss, and of every g_k; r_i, Y, alpha and the weights are powers of two, so the products and quotients with
  them are exact."""
  alpha = alpha_of(temperature)
  pow2 = lambda v: v > 0.0 and math.frexp(v)[0] == 0.5
  if not pow2(alpha):
    return False
  for b in range(len(y)):
    V = [i for i in range(y.shape[1]) if y[b, i] >= 0.0]
    n = len(V)
    if len(set(float(s[b, i]) for i in V)) > 1 or not pow2(float(w[b])):
      return False
    r = (n + 1) / 2.0
    Y = float(sum(y[b, i] for i in V))
    if not (_exact_sum([1.0] + [0.5] * (n - 1)) and pow2(r) and pow2(Y) and _exact_sum([y[b, i] for i in V])):
      return False
    if not _exact_sum([y[b, i] / r for i in V]):
      return False
    c = {i: float(y[b, i]) / ((Y * r) * r) for i in V}
    if any(v != 0.0 and not pow2(v) for v in c.values()):
      return False
    for k in V:
      if not _exact_sum([(c[j] - c[k]) * 0.25 for j in V if j != k]):
        return False
  return True
