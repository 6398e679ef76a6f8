"""Float64 / integer restatement of the list metrics of DESIGN 4.26 (MRR, hits, precision, recall, MAP, DCG, ARP, OPA),
written from the formulas with explicit loops over ranks and pairs, plus the bounds the GPU tests hold the kernel to.
Test infrastructure only: it shares no code with the product.  Orders, ``Entry``, ``bound`` and the input makers come
from tests/listwise_restatement.py.

Formulas (one list; y labels, s scores, V = {i : y_i >= 0}, n = |V|, L the padded width; sigma = V by score descending,
ties by position ascending; r the 0-based rank; k = min(n, topn), topn None = no cut; rel_i = [y_i >= 1]; R = sum_V rel;
c_r = the relevant items at ranks <= r).  Every metric is a per-list value v and a non-negative weight w (v = 0 where
w = 0):
  MRR         v = 1 / (r* + 1), r* the smallest r < k with rel_sigma(r); 0 if none            w = [R > 0]
  hits        v = 1 if some r < k has rel_sigma(r), else 0                                     w = [R > 0]
  precision   v = c_{k-1} / min(topn, L)   (L for topn None: the PADDED width, not n)          w = [R > 0]
  recall      v = c_{k-1} / R                                                                  w = [R > 0]
  MAP         v = (sum_{r < k, rel_sigma(r)} c_r / (r + 1)) / R                                w = [R > 0]
  DCG         v = sum_{r < k} (2^{y_sigma(r)} - 1) / log2(r + 2)                               w = [some y_i > 0]
  ARP         v = sum_V y_sigma(r) (r + 1) / sum_V y                                           w = sum_V y
  OPA         v = C / P, P = #{(i, j) in V^2 : y_i > y_j}, C = #{(i, j) in P : s_i > s_j}      w = P
The result over updates is sum_b q_b w_b v_b / sum_b q_b w_b (q the per-list sample weight, default 1), 0 when the
denominator is 0.

Integer-valued metrics.  MRR, hits, precision, recall and OPA are ONE division of two integers below 2^24 (at most
L^2 = 2^20): both convert to float32 exactly and float32 division is correctly rounded, so the float32 value is
np.float32(num) / np.float32(den) bit for bit -- ``ListMetric.num`` / ``.den`` carry the integers, and the GPU tests
compare bits.  The same holds for their weights (0, 1 or P).

Rounded metrics.  eps = 2^-24; as in tests/listwise_restatement.py a sum of m terms, each with relative error <= u eps,
lies within (m - 1 + u) eps sum|terms| of the exact value for any summation order, a division (and a library call) is
charged 4 ulp, a multiplication or an addition 1, and conversions of integers below 2^24 are exact:
  MAP         a term c_r / (r + 1) is one division of exact integers: u = 4, at most k terms, yardstick the sum of the
              terms (all non-negative); then one division by the exact R:
                  |v~ - v| <= bound(k', sum, 4) / R + 4 eps v          (k' = the relevant ranks below k)
  DCG         the ``_dcg`` entry of tests/listwise_restatement.py as it stands (u = 13, yardstick 2^y / log2(r + 2)).
  ARP         numerator A = sum_V y (r + 1): a term is one multiplication, u = 1, n terms, yardstick A; denominator
              S = sum_V y: exact terms, u = 0, n terms, yardstick S; the ratio
                  |v~ - v| <= b_A / S + v (b_S / S + 4 eps).
              The weight is S.  Where every valid label is an integer and S < 2^24 (labels up to 4: S <= 2^12), S
              and each of its partial sums, in any order, is an integer below 2^24, hence exact in float32: the
              weight's bound is then 0 and the GPU tests compare its bits.  Otherwise the bound is b_S.
Result over updates: a term q w v is two multiplications, a term q w one; each of the two sums runs over B lists in all
(any order, the in-place accumulation across updates included); one division (4 ulp): with non-negative q the result
is within
    (sum_b q_b (w_b e_b + v_b f_b) + result * sum_b q_b f_b) / sum_b q_b w_b + (2 B + 8) eps result
of the exact one, e_b / f_b the per-list bounds on value and weight ((B + 1) + B + 4 first-order roundings, rounded up
to 2 B + 8 for the second-order terms).
"""

import numpy as np

from tests import listwise_restatement as lw
from tests.listwise_restatement import (EPS, FLOOR, SHAPES, Entry, bound, label_order, make_grid_scores,  # noqa: F401
                                        make_labels, make_pow2_weights, make_scores, score_order)

NDCG, DCG, MRR, HITS, PRECISION, RECALL, MAP, ARP, OPA = range(9)
KINDS = {"ndcg": NDCG, "dcg": DCG, "mrr": MRR, "hits": HITS, "precision": PRECISION, "recall": RECALL, "map": MAP,
         "arp": ARP, "opa": OPA}
INTEGER_KINDS = (MRR, HITS, PRECISION, RECALL, OPA)        # one division of two exact integers
ROUNDED_KINDS = (MAP, DCG, ARP)
UNCUT_KINDS = (ARP, OPA)                                   # no topn
MAX_METRICS = 16


class ListMetric:
  """One metric of one list: value and weight in float64, the bounds on both, and for the integer-valued kinds the
  numerator and denominator (value = num / den; den = 1 where the formula gives 0 without a division)."""

  def __init__(self, value, weight, value_bound=0.0, weight_bound=0.0, num=None, den=None):
    self.value, self.weight, self.value_bound, self.weight_bound = value, weight, value_bound, weight_bound
    self.num, self.den = num, den


def _cut(n, topn):
  return n if topn is None else min(n, topn)


def list_metric(kind, y, s, topn=None):
  y = [float(v) for v in y]
  s = [float(v) for v in s]
  L = len(y)
  sigma = score_order(y, s)
  n = len(sigma)
  k = _cut(n, topn)
  rel = [1 if y[i] >= 1.0 else 0 for i in range(L)]
  R = sum(rel[i] for i in sigma)
  has = 1.0 if R > 0 else 0.0
  c = []                                     # c_r
  for r in range(n):
    c.append((c[-1] if c else 0) + rel[sigma[r]])
  ck = c[k - 1] if k > 0 else 0
  if kind == MRR:
    for r in range(k):
      if rel[sigma[r]]:
        return ListMetric(1.0 / (r + 1), has, num=1, den=r + 1)
    return ListMetric(0.0, has, num=0, den=1)
  if kind == HITS:
    hit = 1 if ck > 0 else 0
    return ListMetric(float(hit), has, num=hit, den=1)
  if kind == PRECISION:
    den = L if topn is None else min(topn, L)
    return ListMetric(ck / den if R > 0 else 0.0, has, num=ck if R > 0 else 0, den=den)
  if kind == RECALL:
    return ListMetric(ck / R, has, num=ck, den=R) if R > 0 else ListMetric(0.0, 0.0, num=0, den=1)
  if kind == MAP:
    if R == 0:
      return ListMetric(0.0, 0.0)
    total, terms = 0.0, 0
    for r in range(k):
      if rel[sigma[r]]:
        total += c[r] / (r + 1)
        terms += 1
    v = total / R
    return ListMetric(v, 1.0, float(bound(terms, total, 4.0)) / R + 4.0 * EPS * v)
  if kind == DCG:
    if not any(y[i] > 0.0 for i in sigma):
      return ListMetric(0.0, 0.0)
    e = lw._dcg(sigma, y, topn)
    return ListMetric(e.value, 1.0, float(e.bound))
  if kind == ARP:
    A = S = 0.0
    for r in range(n):
      A += y[sigma[r]] * (r + 1)
      S += y[sigma[r]]
    if not S > 0.0:
      return ListMetric(0.0, 0.0)
    bA, bS = float(bound(n, A, 1.0)), float(bound(n, S, 0.0))
    v = A / S
    integers = all(y[i] == int(y[i]) for i in sigma) and S < 2.0 ** 24
    return ListMetric(v, S, bA / S + v * (bS / S + 4.0 * EPS), 0.0 if integers else bS)
  if kind == OPA:
    P = C = 0
    for i in sigma:
      for j in sigma:
        if y[i] > y[j]:
          P += 1
          if s[i] > s[j]:
            C += 1
    return ListMetric(C / P, float(P), num=C, den=P) if P > 0 else ListMetric(0.0, 0.0, num=0, den=1)
  if kind == NDCG:
    v, counted, b = lw.list_ndcg(y, s, topn)
    return ListMetric(v, counted, b)
  raise ValueError(kind)


class BatchMetric:
  """``list_metric`` over the rows of [B, L] arrays: arrays of values, weights and bounds; ``f32`` the float32 values
  of the integer-valued kinds, ``np.float32(num) / np.float32(den)``."""

  def __init__(self, kind, y, s, topn=None):
    rows = [list_metric(kind, y[b], s[b], topn) for b in range(len(y))]
    self.value = np.array([r.value for r in rows])
    self.weight = np.array([r.weight for r in rows])
    self.value_bound = np.array([r.value_bound for r in rows])
    self.weight_bound = np.array([r.weight_bound for r in rows])
    self.f32 = None
    if kind in INTEGER_KINDS:
      self.num = np.array([r.num for r in rows], dtype=np.int64)
      self.den = np.array([r.den for r in rows], dtype=np.int64)
      assert self.num.max(initial=0) < 2 ** 24 and self.den.max(initial=1) < 2 ** 24 and self.den.min(initial=1) >= 1
      self.f32 = self.num.astype(np.float32) / self.den.astype(np.float32)


def metric_result(kind, batches, topn=None):
  """Metric result over several (y, s, q or None) updates: (value, bound); the docstring above has the derivation."""
  tot = cnt = err_tot = err_cnt = 0.0
  nb = 0
  for y, s, q in batches:
    m = BatchMetric(kind, y, s, topn)
    q = np.ones(len(m.value)) if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    assert (q >= 0).all()
    tot += float(np.sum(q * m.weight * m.value))
    cnt += float(np.sum(q * m.weight))
    err_tot += float(np.sum(q * (m.weight * m.value_bound + m.value * m.weight_bound)))
    err_cnt += float(np.sum(q * m.weight_bound))
    nb += len(m.value)
  if not cnt > 0.0:
    return 0.0, 0.0
  v = tot / cnt
  return v, (err_tot + abs(v) * err_cnt) / cnt + (2.0 * nb + 8.0) * EPS * abs(v)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_sparse_binary_labels(B, L, seed):
  """Labels in {-1, 0, 1} with the padding of ``make_labels``: about one relevant item per list -- one valid position
  set to 1 in three lists out of four, a second one in one list out of four -- so some lists have none."""
  rng = np.random.RandomState(seed + 5)
  y = np.where(make_labels(B, L, seed) >= 0.0, 0.0, -1.0).astype(np.float32)
  for b in range(B):
    valid = np.flatnonzero(y[b] >= 0.0)
    draws = rng.randint(0, 4, size=2)
    if len(valid) and draws[0] != 0:
      y[b, valid[rng.randint(len(valid))]] = 1.0
      if draws[1] == 0:
        y[b, valid[rng.randint(len(valid))]] = 1.0
  return y


def make_half_labels(B, L, seed):
  """``make_labels`` with every 4 replaced by 0.5: not relevant (0.5 < 1), but a positive gain and a positive weight in
  DCG, ARP and OPA."""
  y = make_labels(B, L, seed)
  y[y == 4.0] = 0.5
  return y
