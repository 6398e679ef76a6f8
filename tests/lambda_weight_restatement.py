"""Float64 restatement of the pairwise losses with LambdaRank / LambdaLoss pair weights, written from the
formulas with explicit loops over ranks and pairs, plus the error bound the GPU tests hold the kernels to.  Test
infrastructure only: it shares no code with the product (it imports the helpers of tests/listwise_restatement.py).

Formulas (one list; y labels, s scores, V = {i : y_i >= 0}, n = |V|; topn a positive integer or None, normalized,
mu = smooth_fraction in [0, 1]):
  ranks      r_i in 1 .. n: the rank of valid item i by score descending, ties by position ascending (score_order)
  gain       g_i = 2^{y_i} - 1;  G_i = g_i, or g_i / IDCG when normalized,
             IDCG = sum_{r <= min(n, topn)} (2^{y_pi(r)} - 1) / log2(r + 1), pi = label_order; IDCG <= 0: every weight 0
  discount   D0(r) = 1 / log2(r + 1);  D(r) = D0(r) for r <= topn (or topn None), else 0
  weight     for (i, j) in P = {(i, j) in V^2 : y_i > y_j}, delta = |r_i - r_j|:
             v = |D(r_i) - D(r_j)|,  u = |D0(delta) - D0(delta + 1)|,  c = (1 - mu) v + mu u,  w_ij = |G_i - G_j| c,
             and w_ij = 0 when topn is given and min(r_i, r_j) > topn
  loss       l = sum_P w_ij phi(s_i - s_j), phi as in tests/listwise_restatement.py (logistic or hinge)
  gradient   dl/ds_k = sum_{(k, j) in P} w_kj phi'(s_k - s_j) - sum_{(i, k) in P} w_ik phi'(s_i - s_k)   (w constant)

Ranks are integers obtained from exact comparisons of the float32 scores, so they carry no error: the kernel and this
file, on the same float32 inputs, agree on them exactly (mu is used as the float32 number the kernel receives).

The bound.  As in tests/listwise_restatement.py: eps = 2^-24, an output that is a sum of n terms t_k, each computed with
an absolute error of at most e_k eps, is within  eps ((n - 1) sum |t_k| + sum e_k)  of the exact value for ANY
summation order; every library call (exp2f, log2f, expf, log1pf) and every division is charged 4 ulp, every addition,
subtraction and multiplication 1, all to first order in eps.  What is new is the error of the weight, which is an
ABSOLUTE error (the factors are differences, so their errors are sized by the magnitudes that were subtracted, not by
the difference).  In units of eps:
  gain       2^y: exp2f, 4; the subtraction of 1 rounds once more and cancels for small y, so the error is sized by
             2^y, not by g (the NDCG bound's argument):           E(g_i) = 5 2^{y_i}
  IDCG       a sum of k = min(n, topn) terms (2^y - 1) / log2(r + 1), each 13 ulp of 2^y / log2(r + 1) (exp2f,
             subtraction, log2f, division; tests/listwise_restatement.py), in any order:
                                                                  rho = (k - 1 + 13) (sum_r 2^{y_pi(r)} / log2(r + 1)) / IDCG
             is its RELATIVE error.  Every gain of the list is divided by the SAME rounded IDCG~, so that error is a
             common factor of G_i - G_j and scales the difference, not the two magnitudes; what is sized by the
             magnitudes is each quotient's own part, the gain's error and the division:
                                                                  E(G_i) = 5 2^{y_i} / IDCG + 4 |G_i|
             (not normalized: E(G_i) = E(g_i), rho = 0).
  |G_i - G_j|                                                     E(dG) = E(G_i) + E(G_j) + (1 + rho) |G_i - G_j|
  discount   log2f of an exact integer, a division: 8 ulp of D0(r); a discount cut to 0 is exact.
             v:  E(v) = 8 (D(r_i) + D(r_j)) + v;     u:  E(u) = 8 (D0(delta) + D0(delta + 1)) + u
  c          1 - mu rounds once, each product once, the sum once: at most 3 c on top of the inherited errors:
                                                                  E(c) = (1 - mu) E(v) + mu E(u) + 3 c
             (the mu = 0 kernels form c = v directly; the line above covers them).
  w          one product:                                         E(w) = E(dG) c + |G_i - G_j| E(c) + w
  term       w phi(x): phi carries u_phi ulp of its yardstick Y (tests/listwise_restatement.py: logistic u_phi = 10,
             Y = phi(x) (1 + |x|); hinge u_phi = 2, Y = 1 + |x| for an active pair or one within 1e-6 of the kink),
             then one product:                                    e = E(w) Y + (u_phi + 1) w Y,  |term| <= w Y
             Gradient terms w phi'(x) likewise (logistic: u = 10, Y = |phi'(x)| (1 + |x|); hinge: phi' exact, Y = |phi'|).
An ``Entry`` (tests/listwise_restatement.py) is (value, n, yard, u) with bound (n - 1 + u) eps yard.  Here yard =
sum w Y over the entry's terms and u = (sum e) / yard, the yardstick-weighted mean of the terms' error counts, so that
``Entry.bound`` is exactly eps ((n - 1) yard + sum e).  u is per entry, not one constant per kind: it grows where the
gains cancel (equal-looking labels far down a long list) and the tests print it.  The absolute floor 2^-126 of that file
applies as well.

``list_loss`` is the definition: scalar float64, explicit loops over ranks and pairs.  ``batch_loss`` evaluates the same
expressions one ROW of pairs (i, .) at a time as float64 numpy vectors, so that the reference of a [67, 257] batch takes
a second, not minutes; tests/test_lambda_weight_host.py holds it to ``list_loss`` (value, yardstick and u) on random
lists."""

import collections
import math

import numpy as np

from tests import listwise_restatement as lw

EPS, FLOOR, Entry = lw.EPS, lw.FLOOR, lw.Entry
PAIRWISE_LOGISTIC, PAIRWISE_HINGE = lw.PAIRWISE_LOGISTIC, lw.PAIRWISE_HINGE
KINDS = {"pairwise_logistic": PAIRWISE_LOGISTIC, "pairwise_hinge": PAIRWISE_HINGE}

Config = collections.namedtuple("Config", "topn normalized mu")
Config.__new__.__defaults__ = (None, False, 0.0)


def d0(r):
  return 1.0 / math.log2(r + 1.0)


def ranks(y, s):
  """{position: rank in 1 .. n} of the valid items."""
  return {i: r + 1 for r, i in enumerate(lw.score_order(y, s))}


class Weights:
  """Per-item quantities of one list's weights and ``pair(i, j)`` -> (w_ij, E(w_ij) in eps)."""

  def __init__(self, y, s, cfg):
    self.cfg = cfg
    self.mu = float(np.float32(cfg.mu))
    self.rank = ranks(y, s)
    n = len(self.rank)
    topn = cfg.topn
    self.D = {i: (d0(r) if topn is None or r <= topn else 0.0) for i, r in self.rank.items()}
    self.G, self.EG = {}, {}
    self.zero = False
    idcg, rho = 1.0, 0.0
    if cfg.normalized:
      pi = lw.label_order(y)
      k = n if topn is None else min(n, topn)
      idcg = yard = 0.0
      for r in range(1, k + 1):
        idcg += (2.0 ** y[pi[r - 1]] - 1.0) / math.log2(r + 1.0)
        yard += 2.0 ** y[pi[r - 1]] / math.log2(r + 1.0)
      self.zero = not idcg > 0.0
      if not self.zero:
        rho = (max(k - 1, 0) + 13.0) * yard / idcg
    self.idcg, self.rho = idcg, rho
    for i in self.rank:
      if self.zero:
        self.G[i], self.EG[i] = 0.0, 0.0
      elif cfg.normalized:
        self.G[i] = (2.0 ** y[i] - 1.0) / idcg
        self.EG[i] = 5.0 * 2.0 ** y[i] / idcg + 4.0 * abs(self.G[i])
      else:
        self.G[i] = 2.0 ** y[i] - 1.0
        self.EG[i] = 5.0 * 2.0 ** y[i]

  def pair(self, i, j):
    ri, rj = self.rank[i], self.rank[j]
    topn = self.cfg.topn
    if self.zero or (topn is not None and min(ri, rj) > topn):
      return 0.0, 0.0
    dg = abs(self.G[i] - self.G[j])
    e_dg = self.EG[i] + self.EG[j] + (1.0 + self.rho) * dg
    v = abs(self.D[i] - self.D[j])
    e_v = 8.0 * (self.D[i] + self.D[j]) + v
    delta = abs(ri - rj)
    u = abs(d0(delta) - d0(delta + 1))
    e_u = 8.0 * (d0(delta) + d0(delta + 1)) + u
    c = (1.0 - self.mu) * v + self.mu * u
    e_c = (1.0 - self.mu) * e_v + self.mu * e_u + 3.0 * c
    w = dg * c
    return w, e_dg * c + dg * e_c + w


def pair_weights(y, s, cfg=Config()):
  """{(i, j): w_ij} over P, by the explicit loops."""
  y = [float(v) for v in y]
  s = [float(v) for v in s]
  wt = Weights(y, s, cfg)
  V = lw._valid(y)
  return {(i, j): wt.pair(i, j)[0] for i in V for j in V if y[i] > y[j]}


def _entry(val, n, yard, err):
  """Entry with bound eps ((n - 1) yard + err): u = err / yard."""
  yard = np.asarray(yard, dtype=np.float64)
  u = np.divide(err, yard, out=np.zeros_like(yard), where=yard > 0.0)
  return Entry(val, n, yard, u)


def list_loss(kind, y, s, cfg=Config()):
  """One list, explicit loops: (Entry of the loss, Entry of the gradient [L])."""
  y = [float(v) for v in y]
  s = [float(v) for v in s]
  L = len(y)
  V = lw._valid(y)
  wt = Weights(y, s, cfg)
  logistic = kind == PAIRWISE_LOGISTIC
  u_val = 10.0 if logistic else 2.0
  u_grad = 10.0 if logistic else 0.0
  val = yard = err = 0.0
  cnt = 0
  g, gn, gy, ge = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
  for i in V:
    for j in V:
      if y[i] > y[j]:
        w, e_w = wt.pair(i, j)
        x = s[i] - s[j]
        p = lw._phi(kind, x)
        d = lw._dphi(kind, x)
        Y = lw._pair_yard(kind, x, p)
        val += w * p
        yard += w * Y
        err += e_w * Y + (u_val + 1.0) * w * Y
        cnt += 1
        Yd = abs(d) * (1.0 + abs(x)) if logistic else abs(d)
        g[i] += w * d
        g[j] -= w * d
        for k in (i, j):
          gn[k] += 1
          gy[k] += w * Yd
          ge[k] += e_w * Yd + (u_grad + 1.0) * w * Yd
  return _entry(val, cnt, yard, err), _entry(g, gn, gy, ge)


def _rows(kind, y, s, cfg):
  """list_loss with the pairs (i, .) of one item as float64 vectors over the valid items."""
  L = len(y)
  V = np.array(lw._valid(y), dtype=np.int64)
  n = len(V)
  g, gn, gy, ge = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
  if n == 0:
    return (0.0, 0, 0.0, 0.0), (g, gn, gy, ge)
  wt = Weights([float(v) for v in y], [float(v) for v in s], cfg)
  yv = np.asarray(y, dtype=np.float64)[V]
  sv = np.asarray(s, dtype=np.float64)[V]
  rk = np.array([wt.rank[i] for i in V], dtype=np.int64)
  D = np.array([wt.D[i] for i in V])
  G = np.array([wt.G[i] for i in V])
  EG = np.array([wt.EG[i] for i in V])
  tab = np.array([0.0] + [d0(r) for r in range(1, n + 2)])      # tab[r] = D0(r)
  mu, topn = wt.mu, cfg.topn
  logistic = kind == PAIRWISE_LOGISTIC
  u_val = 10.0 if logistic else 2.0
  u_grad = 10.0 if logistic else 0.0
  val = yard = err = 0.0
  cnt = 0
  a, an, ay, ae = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
  for i in range(n):
    m = yv[i] > yv
    if not m.any():
      continue
    dg = np.abs(G[i] - G)
    e_dg = EG[i] + EG + (1.0 + wt.rho) * dg
    v = np.abs(D[i] - D)
    e_v = 8.0 * (D[i] + D) + v
    delta = np.abs(rk[i] - rk)
    u = np.abs(tab[delta] - tab[delta + 1])
    e_u = 8.0 * (tab[delta] + tab[delta + 1]) + u
    c = (1.0 - mu) * v + mu * u
    e_c = (1.0 - mu) * e_v + mu * e_u + 3.0 * c
    w = dg * c
    e_w = e_dg * c + dg * e_c + w
    dead = ~m
    if wt.zero:
      dead = np.ones(n, dtype=bool)
    elif topn is not None:
      dead = dead | (np.minimum(rk[i], rk) > topn)
    w = np.where(dead, 0.0, w)
    e_w = np.where(dead, 0.0, e_w)
    x = sv[i] - sv
    ax = np.abs(x)
    if logistic:
      e = np.exp(-ax)
      p = np.maximum(-x, 0.0) + np.log1p(e)
      d = np.where(x >= 0.0, -e / (1.0 + e), -1.0 / (1.0 + e))
      Y = p * (1.0 + ax)
      Yd = np.abs(d) * (1.0 + ax)
    else:
      p = np.maximum(0.0, 1.0 - x)
      d = np.where(x < 1.0, -1.0, 0.0)
      Y = np.where(x < 1.0 + 1e-6, 1.0 + ax, 0.0)
      Yd = np.abs(d)
    val += float(np.sum(w * p))
    yard += float(np.sum(w * Y))
    err += float(np.sum(e_w * Y + (u_val + 1.0) * w * Y))
    k = int(m.sum())
    cnt += k
    wd = w * d
    a[i] += float(np.sum(wd))
    a -= wd
    an[i] += k
    an += m
    ay[i] += float(np.sum(w * Yd))
    ay += w * Yd
    t = e_w * Yd + (u_grad + 1.0) * w * Yd
    ae[i] += float(np.sum(t))
    ae += t
  g[V], gn[V], gy[V], ge[V] = a, an, ay, ae
  return (val, cnt, yard, err), (g, gn, gy, ge)


def batch_loss(kind, y, s, cfg=Config()):
  """[B, L] arrays -> (Entry of the per-list losses [B], Entry of the gradients [B, L]); u is per entry."""
  y = np.asarray(y, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  B, L = y.shape
  lo = np.zeros((4, B))
  gr = np.zeros((4, B, L))
  for b in range(B):
    l4, g4 = _rows(kind, y[b], s[b], cfg)
    lo[:, b] = l4
    for k in range(4):
      gr[k, b] = g4[k]
  return _entry(lo[0], lo[1], lo[2], lo[3]), _entry(gr[0], gr[1], gr[2], gr[3])


def implied_order(y, s):
  """Per list: the valid positions in rank order (the ranks the kernel must have used)."""
  return [lw.score_order([float(v) for v in y[b]], [float(v) for v in s[b]]) for b in range(len(y))]


# ---- the configurations and shapes of tests/test_lambda_weight_gpu.py --------------------------------------------------
LENGTHS = (1, 2, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130, 257, 1024)
SHAPES = tuple((b, l) for l in LENGTHS for b in ((3,) if l == 1024 else (1, 3, 67)))


def configs(L):
  """name -> Config: NDCG, DCG, topn in {1, 3, L, L + 5} and mu in {0.25, 1} (those six on the NDCG weight), and one
  that combines a cut with a smooth fraction."""
  out = {"ndcg": Config(None, True, 0.0), "dcg": Config(None, False, 0.0)}
  for name, topn in (("topn1", 1), ("topn3", 3), ("topnL", L), ("topnL+5", L + 5)):
    out[name] = Config(topn, True, 0.0)
  out["mu0.25"] = Config(None, True, 0.25)
  out["mu1"] = Config(None, True, 1.0)
  out["dcg_topn3_mu0.25"] = Config(3, False, 0.25)      # the cut inside the smooth pair loop, on raw gains
  return out


CONFIG_NAMES = tuple(configs(1))
