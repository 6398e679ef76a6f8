"""float64 NumPy restatement of the multi-head (max-sim) Retrieval loss, its gradients and the multi-head top-K
(test infrastructure only).

Follows ``tasks/retrieval.py:172-210`` of the reference for queries ``[B, H, D]``:

    M_bc = max_h q_bh . c_c                          (:173-176, the max on the raw dot products)
    S_bc = M_bc / T - log clip(p_c, 1e-6, 1) + MIN_FLOAT [accidental hit] ; MIN_FLOAT where the mask is off
    loss = sum_b w_b (logsumexp_c S_bc - S_bb)
    G_bc = w_b (softmax(S_b)_c - [b == c]) / T       (0 where masked)
    dQ_bh = sum_c [h == h*(b, c)] G_bc c_c ,  dC_c = sum_b G_bc q_{b, h*(b, c)}

with ``h*(b, c)`` the LOWEST head attaining the max (``argmax``'s first-index rule, which is also what
``torch.max(dim)`` back-propagates to).  Inputs are taken as they come (float64 inputs stay float64, so the
functions can be differentiated numerically).
"""

import numpy as np

from oracle import retrieval as o_ret
from oracle import topk as o_topk

MIN_FLOAT = float(o_ret.MIN_FLOAT)


def head_dots(q3, c):
  """``[B, H, C]`` dot products in float64."""
  return np.einsum("bhd,cd->bhc", np.asarray(q3, dtype=np.float64), np.asarray(c, dtype=np.float64))


def winners(q3, c):
  """``(M [B, C], h* [B, C])``: the max over heads and the lowest head attaining it."""
  dots = head_dots(q3, c)
  return dots.max(axis=1), dots.argmax(axis=1)


def logits(q3, c, temperature=None, candidate_sampling_probability=None, candidate_ids=None, score_mask=None):
  m, _ = winners(q3, c)
  nq, nc = m.shape
  s = m if temperature is None else m / float(temperature)
  if candidate_sampling_probability is not None:                         # loss.py:153-158
    p = np.clip(np.asarray(candidate_sampling_probability, dtype=np.float32), 1e-6, 1.0)
    s = s - np.log(p.astype(np.float64))[None, :]
  if candidate_ids is not None:                                          # loss.py:117-147
    ids = np.asarray(candidate_ids)
    dup = (ids[:nq, None] == ids[None, :]).astype(np.float64) - np.eye(nq, nc)
    s = s + dup * MIN_FLOAT
  if score_mask is not None:                                             # retrieval.py:202-203
    s = np.where(np.asarray(score_mask, dtype=bool), s, MIN_FLOAT)
  return s


def _softmax(s):
  z = s - s.max(axis=1, keepdims=True)
  e = np.exp(z)
  return e / e.sum(axis=1, keepdims=True), s.max(axis=1) + np.log(e.sum(axis=1))


def loss(q3, c, sample_weight=None, **kw):
  s = logits(q3, c, **kw)
  _, lse = _softmax(s)
  per_row = lse - s[np.arange(s.shape[0]), np.arange(s.shape[0])]
  if sample_weight is not None:
    per_row = per_row * np.asarray(sample_weight, dtype=np.float64).reshape(-1)
  return float(per_row.sum())


def loss_grads(q3, c, sample_weight=None, temperature=None, candidate_sampling_probability=None,
               candidate_ids=None, score_mask=None, return_yardsticks=False):
  """``(dQ [B, H, D], dC [C, D])`` in float64; with ``return_yardsticks`` also the scale a floating-point error of
  each entry is measured in, built like ``oracle.retrieval.loss_grads(return_yardsticks=True)``: the sum of the
  absolute values of the entry's terms, each probability carrying the relative error ``A_bc + sum_c p_bc A_bc`` of
  its logit and its row's logsumexp, ``A_bc = sum_d |q_{b,h*,d}| |c_cd| / |T|`` over the WINNING head's row."""
  q = np.asarray(q3, dtype=np.float64)
  cc = np.asarray(c, dtype=np.float64)
  nq, heads, _ = q.shape
  nc = cc.shape[0]
  s = logits(q, cc, temperature, candidate_sampling_probability, candidate_ids, score_mask)
  _, hstar = winners(q, cc)
  p, _ = _softmax(s)
  labels = np.eye(nq, nc)
  g = p - labels
  t_abs = abs(float(temperature)) if temperature is not None else 1.0
  onehot = (np.arange(heads)[None, :, None] == hstar[:, None, :]).astype(np.float64)      # [B, H, C]
  cond = np.einsum("bhc,bhd,cd->bc", onehot, np.abs(q), np.abs(cc)) / t_abs
  cond = cond + (p * cond).sum(axis=1, keepdims=True)
  ga = p * (1.0 + cond) + labels
  if sample_weight is not None:
    w = np.asarray(sample_weight, dtype=np.float64).reshape(-1, 1)
    g, ga = g * w, ga * np.abs(w)
  if score_mask is not None:
    on = np.asarray(score_mask, dtype=bool)
    g, ga = np.where(on, g, 0.0), np.where(on, ga, 0.0)
  if temperature is not None:
    g, ga = g / float(temperature), ga / t_abs
  dq = np.einsum("bhc,bc,cd->bhd", onehot, g, cc)
  dc = np.einsum("bhc,bc,bhd->cd", onehot, g, q)
  if return_yardsticks:
    return (dq, dc, np.einsum("bhc,bc,cd->bhd", onehot, ga, np.abs(cc)),
            np.einsum("bhc,bc,bhd->cd", onehot, ga, np.abs(q)))
  return dq, dc


def head_gap_guard(q3, c):
  """``(smallest gap between a pair's two best heads, 64 * d * 2^-24 * max sum_d |q||c|)``: when the gap is
  above the bound, an f32 evaluation of the dot products in any summation order picks the float64 winners."""
  q = np.asarray(q3, dtype=np.float64)
  cc = np.asarray(c, dtype=np.float64)
  if q.shape[1] < 2:
    return np.inf, 0.0
  dots = np.sort(head_dots(q, cc), axis=1)
  gap = float((dots[:, -1, :] - dots[:, -2, :]).min())
  mag = float(np.einsum("bhd,cd->bhc", np.abs(q), np.abs(cc)).max())
  return gap, 64.0 * q.shape[2] * 2.0 ** -24 * mag


def head_scores(q3, c):
  """``[B, H, N]`` float32 scores of every head as the d-ordered fma chain of ``oracle.topk.scores``."""
  q = np.ascontiguousarray(q3, dtype=np.float32)
  nq, heads, d = q.shape
  return o_topk.scores(q.reshape(nq * heads, d), c).reshape(nq, heads, -1)


def topk(q3, c, k):
  """Top-k of ``max_h`` of the heads' scores under (score descending, row ascending)."""
  return o_topk.top_k(head_scores(q3, c).max(axis=1), k)
