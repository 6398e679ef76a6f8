"""NumPy restatement of hard-negative mining and the batch metric over ADJUSTED in-batch logits (test
infrastructure only).

Follows ``tasks/retrieval.py:178-210, 228-232`` and ``layers/loss.py:91-109`` of the reference for 2-D queries:

    S_bc = (q_b . c_c) / T - log clip(p_c, 1e-6, 1) [+ MIN_FLOAT if ids_c == ids_b, c != b] ; MIN_FLOAT where !mask
    kept set of row b = its positive and the n = min(num_hard_negatives, C - 1) largest negatives, equal values to
                        the lower column: the first n + 1 columns of a stable argsort of -(S + labels * MAX_FLOAT)
    keep(b, c) = (c == b) || S_bc > tau_b || (S_bc == tau_b && c <= cut_b)
    loss = sum_b w_b (logsumexp_{c kept} S_bc - S_bb) ;  G_bc = w_b (softmax_kept(S_b)_c - [b == c]) / T
    count_b = #{c != b kept : S_bc > S_bb}

``logits(..., exact_f32=True)`` forms S with float32 operations in the order of the device (dot, IEEE division,
subtraction, MIN_FLOAT addend, mask, -0 -> +0): for integer-valued embeddings the dot is exact in any summation
order, so the result is what the kernels hold bit for bit.  The float64 form serves random floats behind
``boundary_gap_guard``.
"""

import numpy as np

from oracle import retrieval as o_ret

MIN_FLOAT = np.float32(o_ret.MIN_FLOAT)
MAX_FLOAT = np.float32(o_ret.MAX_FLOAT)
CUT_ALL = np.iinfo(np.int64).max


def log_correction(candidate_sampling_probability):
  """``log clip(p, 1e-6, 1)`` in float32 (loss.py:157-158): what the C ABI takes."""
  return np.log(np.clip(np.asarray(candidate_sampling_probability, dtype=np.float32), 1e-6, 1.0)).astype(np.float32)


def logits(q, c, temperature=None, candidate_sampling_probability=None, candidate_ids=None, score_mask=None,
           log_corr=None, exact_f32=False):
  """``[B, C]`` adjusted logits; ``log_corr`` gives ``log clip(p)`` directly instead of ``p``."""
  ft = np.float32 if exact_f32 else np.float64
  dots = np.asarray(q, dtype=np.float64) @ np.asarray(c, dtype=np.float64).T
  s = dots.astype(ft)
  nq, nc = s.shape
  if temperature is not None:
    s = (s / ft(temperature)).astype(ft)
  if candidate_sampling_probability is not None:
    log_corr = log_correction(candidate_sampling_probability)
  if log_corr is not None:
    s = (s - np.asarray(log_corr, dtype=np.float32).astype(ft)[None, :]).astype(ft)
  if candidate_ids is not None:
    ids = np.asarray(candidate_ids)
    hit = (ids[:nq, None] == ids[None, :]) & ~np.eye(nq, nc, dtype=bool)
    s = np.where(hit, (s + ft(MIN_FLOAT)).astype(ft), s)
  if score_mask is not None:
    s = np.where(np.asarray(score_mask, dtype=bool), s, ft(MIN_FLOAT))
  return (s + ft(0.0)).astype(ft)


def kept_columns(s, num_hard_negatives):
  """The columns ``hard_negative_mining`` keeps, positive first, then by descending logit (stable)."""
  nq, nc = s.shape
  n = min(int(num_hard_negatives), nc - 1)
  keyed = s.astype(np.float64) + np.eye(nq, nc) * float(MAX_FLOAT)
  return np.argsort(-keyed, axis=1, kind="stable")[:, :n + 1]


def kept_set(s, num_hard_negatives=None):
  """Boolean ``[B, C]``; ``None`` keeps everything."""
  if num_hard_negatives is None:
    return np.ones(s.shape, dtype=bool)
  keep = np.zeros(s.shape, dtype=bool)
  np.put_along_axis(keep, kept_columns(s, num_hard_negatives), True, axis=1)
  return keep


def tau_cut(s, num_hard_negatives):
  """``(tau [B] of s.dtype, cut [B] int64)`` of the kept set."""
  nq, nc = s.shape
  keep = kept_set(s, num_hard_negatives)
  tau = np.full(nq, np.inf, dtype=s.dtype)
  cut = np.full(nq, -1, dtype=np.int64)
  for b in range(nq):
    neg = keep[b].copy()
    neg[b] = False
    if not neg.any():
      continue
    tau[b] = s[b, neg].min()
    ties = (s[b] == tau[b])
    ties[b] = False
    taken = ties & neg
    cut[b] = CUT_ALL if taken.sum() == ties.sum() else int(np.flatnonzero(taken).max())
  return tau, cut


def keep_from_tau_cut(s, tau, cut):
  nq, nc = s.shape
  cols = np.arange(nc)[None, :]
  return (cols == np.arange(nq)[:, None]) | (s > tau[:, None]) | ((s == tau[:, None]) & (cols <= cut[:, None]))


def _softmax_kept(s, keep):
  z = np.where(keep, s.astype(np.float64), -np.inf)
  m = z.max(axis=1, keepdims=True)
  e = np.exp(z - m)
  tot = e.sum(axis=1, keepdims=True)
  return e / tot, (m + np.log(tot))[:, 0], m[:, 0], np.log(tot)[:, 0]


def loss(s, keep, sample_weight=None):
  """float64; ``(max - pos) + log(sum)`` so that a row of MIN_FLOATs gives ``log(kept)`` exactly."""
  _, _, m, logtot = _softmax_kept(s, keep)
  pos = s[np.arange(s.shape[0]), np.arange(s.shape[0])].astype(np.float64)
  per_row = (m - pos) + logtot
  if sample_weight is not None:
    per_row = per_row * np.asarray(sample_weight, dtype=np.float64).reshape(-1)
  return float(per_row.sum())


def loss_grads(q, c, s, keep, sample_weight=None, temperature=None, score_mask=None):
  """``(dQ, dC, yardstick of dQ, yardstick of dC)`` in float64, the yardsticks built like
  ``multihead_restatement.loss_grads``: the sum of the absolute values of an entry's terms, each probability carrying
  the relative error ``A_bc + sum_c p_bc A_bc`` of its logit and its row's logsumexp, ``A_bc = sum_d |q_bd| |c_cd| / |T|``."""
  q = np.asarray(q, dtype=np.float64)
  cc = np.asarray(c, dtype=np.float64)
  nq, nc = s.shape
  p, _, _, _ = _softmax_kept(s, keep)
  labels = np.eye(nq, nc)
  g = p - labels
  t_abs = abs(float(temperature)) if temperature is not None else 1.0
  cond = np.abs(q) @ np.abs(cc).T / t_abs
  cond = cond + (p * cond).sum(axis=1, keepdims=True)
  ga = p * (1.0 + cond) + labels
  if sample_weight is not None:
    w = np.asarray(sample_weight, dtype=np.float64).reshape(-1, 1)
    g, ga = g * w, ga * np.abs(w)
  on = keep if score_mask is None else keep & np.asarray(score_mask, dtype=bool)
  g, ga = np.where(on, g, 0.0), np.where(on, ga, 0.0)
  if temperature is not None:
    g, ga = g / float(temperature), ga / t_abs
  return g @ cc, g.T @ q, ga @ np.abs(cc), ga.T @ np.abs(q)


def pair_gradient(s, keep, sample_weight=None, temperature=None, score_mask=None):
  """``G [B, C]`` in float64 (for the tests that count its non-zero entries)."""
  nq, nc = s.shape
  p, _, _, _ = _softmax_kept(s, keep)
  g = p - np.eye(nq, nc)
  if sample_weight is not None:
    g = g * np.asarray(sample_weight, dtype=np.float64).reshape(-1, 1)
  on = keep if score_mask is None else keep & np.asarray(score_mask, dtype=bool)
  return np.where(on, g, 0.0) / (float(temperature) if temperature is not None else 1.0)


def rank_counts(s, keep):
  """``count_b`` and ``isfinite(S_bb)``."""
  nq, nc = s.shape
  pos = s[np.arange(nq), np.arange(nq)]
  above = keep & (s > pos[:, None]) & ~np.eye(nq, nc, dtype=bool)
  return above.sum(axis=1), np.isfinite(pos)


def top_k_hits(s, keep, k):
  counts, finite = rank_counts(s, keep)
  return ((counts < k) & finite).astype(np.float32)


def boundary_gap_guard(q, c, s, num_hard_negatives, temperature=None):
  """``(gap [B], bound)``: per row the gap between its n-th and (n + 1)-th largest negative logit (inf when every
  negative is kept or none is), against ``64 * d * 2^-24 * max sum_d |q||c| / |T|``: above the bound an f32
  evaluation of the dot products in any summation order keeps the float64 kept set."""
  q = np.asarray(q, dtype=np.float64)
  cc = np.asarray(c, dtype=np.float64)
  nq, nc = s.shape
  n = min(int(num_hard_negatives), nc - 1)
  t_abs = abs(float(temperature)) if temperature is not None else 1.0
  bound = 64.0 * q.shape[1] * 2.0 ** -24 * float((np.abs(q) @ np.abs(cc).T).max()) / t_abs
  if n == 0 or n == nc - 1:
    return np.full(nq, np.inf), bound
  neg = np.where(np.eye(nq, nc, dtype=bool), -np.inf, s.astype(np.float64))
  srt = -np.sort(-neg, axis=1)
  return srt[:, n - 1] - srt[:, n], bound


def option_variants(rng, nq, nc):
  """Every logit option alone and all together (the keys are test ids)."""
  w = rng.uniform(0.1, 2.0, size=nq).astype(np.float32)
  p = rng.uniform(0.0, 1.0, size=nc).astype(np.float32)
  p[::7] = 0.0                                          # the 1e-6 clip
  ids = rng.integers(0, max(nc // 2, 2), size=nc)       # duplicates: accidental hits
  mask = rng.uniform(size=(nq, nc)) > 0.1
  mask[np.arange(nq), np.arange(nq)] = True
  return {"plain": dict(), "weights": dict(sample_weight=w), "temperature": dict(temperature=0.7),
          "correction": dict(candidate_sampling_probability=p), "accidental_hits": dict(candidate_ids=ids),
          "mask": dict(score_mask=mask),
          "all": dict(sample_weight=w, temperature=1.3, candidate_sampling_probability=p, candidate_ids=ids,
                      score_mask=mask)}


def logit_options(kw):
  return {k: v for k, v in kw.items() if k != "sample_weight"}


GUARDED_SHAPES = ((70, 333, 48), (96, 96, 128), (300, 300, 64))
GUARDED_NS = (1, 7, 50)
_GUARDED = {}


def guarded_case(nq, nc, d):
  """``(q, c, variants)``: normal embeddings (logits of unit scale) under which EVERY row passes
  ``boundary_gap_guard`` for every variant and every n of ``GUARDED_NS``.  A query whose row misses the guard
  somewhere is drawn again from the same generator (a query touches its own row of logits only) until no row is
  left; the result is a fixed function of the shape.  Computed once per process."""
  key = (nq, nc, d)
  if key in _GUARDED:
    return _GUARDED[key]
  rng = np.random.default_rng(1000 * nq + nc + d)
  q = (rng.normal(size=(nq, d)) / d ** 0.25).astype(np.float32)
  c = (rng.normal(size=(nc, d)) / d ** 0.25).astype(np.float32)
  variants = option_variants(rng, nq, nc)
  for _ in range(500):
    bad = np.zeros(nq, dtype=bool)
    for kw in variants.values():
      s = logits(q, c, **logit_options(kw))
      for n in GUARDED_NS:
        gap, bound = boundary_gap_guard(q, c, s, n, kw.get("temperature"))
        bad |= ~(gap > bound)
    if not bad.any():
      _GUARDED[key] = (q, c, variants)
      return _GUARDED[key]
    q[bad] = (rng.normal(size=(int(bad.sum()), d)) / d ** 0.25).astype(np.float32)
  raise AssertionError(f"no guarded inputs at {key}: rows {np.flatnonzero(bad)[:8]} keep missing the guard")
