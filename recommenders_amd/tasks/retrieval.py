"""The factorized retrieval task on MI355X.

Mirror of ``tensorflow_recommenders/tasks/retrieval.py:29-235``: same constructor and
``call`` arguments.  The default loss -- in-batch sampled softmax, i.e. Keras
``CategoricalCrossentropy(from_logits=True, reduction=SUM)`` on ``labels = eye`` (:86-87,
:185, :210) -- runs as a fused f32-MFMA kernel pair that never materialises the
``[num_queries, num_candidates]`` logits (``tfrs_inbatch_softmax_ce_fwd/_bwd``), with
temperature (:187), sampling-probability correction (:190), accidental-hit removal
(:194-200) and ``score_mask`` (:202) folded into the logit function.

``batch_metrics`` (:228-232) are updated from rank counts -- of the plain dot products
(``TopKCategoricalAccuracy.update_from_embeddings``) or of the adjusted / mined logits the loss saw
(``update_from_adjusted``: the temperature divides there as in the reference).  ``num_hard_negatives`` (:205-208) over
plain dot-product logits takes the fused top-K search (``hard_negative_softmax_loss``); every other hard-negative
configuration of the built-in loss -- a sampling correction, accidental-hit removal, a score mask, batch metrics, any
``num_hard_negatives`` -- takes ``mined_in_batch_softmax_loss``: an exact radix select per row and a keep predicate
inside the streaming kernels (``tfrs_inbatch_mined_*``).  None of these builds the ``[num_queries, num_candidates]``
matrix.  Multi-head (3-D, max-sim) queries (:173-176)
with up to 32 heads take the same fused route (``tfrs_inbatch_softmax_mh_ce_fwd/_bwd``: the max over
heads is taken inside the kernels, the gradient of a pair goes to its lowest maximal head).  What
still needs the explicit matrix -- a user-supplied ``loss`` (its contract IS the matrix), embedding dims above 128,
more queries than candidates, foreign batch-metric classes, and multi-head queries
combined with hard negatives, batch metrics or more than 32 heads -- computes it with the HIP dense
GEMM and then follows the reference's op sequence on that tensor.  ``TFRS_RETRIEVAL_EXPLICIT=1`` (read per call) sends
hard negatives / batch metrics over adjusted logits back to that route: the comparator of tests and
``tools/bench_hard_negatives.py``.

All of the above is ONE decision, taken by the pure function ``pick_routes`` from the facts of a call's configuration:
a ``LossRoute`` (fused 2-D, fused multi-head, top-K hard negatives, mined, matrix cross-entropy, custom loss) and a
``MetricRoute`` (none, rank count on plain dot products, rank count on adjusted logits, matrix).
``Retrieval.forward`` dispatches on the two values and builds the matrix exactly when one of them uses it
(``needs_matrix``); ``tests/test_retrieval_route_host.py`` enumerates the function on the host.
"""

import enum
import os
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from recommenders_amd import _lib
from recommenders_amd import _streams
from recommenders_amd.layers import loss as loss_layers
from recommenders_amd.layers.feature_interaction.dcn import _DenseFn
from recommenders_amd.metrics import factorized_top_k as tfrs_metrics
from recommenders_amd.tasks import base

MIN_FLOAT = float(np.finfo(np.float32).min / 100.0)   # retrieval.py:26


class _InBatchSoftmaxFn(torch.autograd.Function):
  """loss = sum_b w_b (logsumexp_c S_bc - S_bb), gradients wrt both embedding matrices.  Queries ``[B, D]``, or
  ``[B, H, D]``: the same loss on logits ``max_h q_bh . c_c``; the gradient of a (query, candidate) pair flows to the
  lowest head that attains the max."""

  @staticmethod
  def _entry(lib, q, c, name):
    """The C entry point ``name`` for the rank of ``q`` and the shape arguments both families begin with."""
    if q.dim() == 3:
      return getattr(lib, "tfrs_inbatch_softmax_mh_" + name), (q.shape[0], q.shape[1], c.shape[0], q.shape[2])
    return getattr(lib, "tfrs_inbatch_softmax_" + name), (q.shape[0], c.shape[0], q.shape[1])

  @staticmethod
  def _workspace(lib, q, c):
    fn, shape = _InBatchSoftmaxFn._entry(lib, q, c, "workspace_bytes")
    return torch.empty((fn(*shape),), dtype=torch.uint8, device=q.device)

  @staticmethod
  def forward(ctx, q, c, sample_weight, inv_t, log_corr, cand_ids, score_mask):
    lib = _lib.load()
    q = q.contiguous()
    c = c.contiguous()
    nq = q.shape[0]
    ws = _InBatchSoftmaxFn._workspace(lib, q, c)
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    lse = torch.empty((nq,), dtype=torch.float32, device=q.device)
    pos = torch.empty((nq,), dtype=torch.float32, device=q.device)
    fwd, shape = _InBatchSoftmaxFn._entry(lib, q, c, "ce_fwd")
    _lib.check(fwd(
        _lib.ptr(q), _lib.ptr(c), *shape, _lib.ptr(sample_weight), float(inv_t),
        _lib.ptr(log_corr), _lib.ptr(cand_ids), _lib.ptr(score_mask), _lib.ptr(loss),
        _lib.ptr(lse), _lib.ptr(pos), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    # 2-D: the workspace keeps the forward's operand images for the backward (split-fp16 path)
    ctx.save_for_backward(q, c, sample_weight, log_corr, cand_ids, score_mask, lse, ws if q.dim() == 2 else None)
    ctx.inv_t = float(inv_t)
    return loss

  @staticmethod
  def backward(ctx, gloss):
    q, c, sample_weight, log_corr, cand_ids, score_mask, lse, ws = ctx.saved_tensors
    lib = _lib.load()
    dq = torch.empty_like(q)
    dc = torch.empty_like(c)
    g = gloss.to(torch.float32).contiguous()
    reuse = ()
    if ws is None:                                                      # multi-head: a fresh workspace
      ws = _InBatchSoftmaxFn._workspace(lib, q, c)
    else:
      reuse = (0 if os.environ.get("TFRS_SOFTMAX_NO_REUSE") else 1,)
    bwd, shape = _InBatchSoftmaxFn._entry(lib, q, c, "ce_bwd")
    _lib.check(bwd(
        _lib.ptr(q), _lib.ptr(c), *shape, _lib.ptr(sample_weight), ctx.inv_t,
        _lib.ptr(log_corr), _lib.ptr(cand_ids), _lib.ptr(score_mask), _lib.ptr(lse),
        _lib.ptr(g), _lib.ptr(dq), _lib.ptr(dc), _lib.ptr(ws), ws.numel(), *reuse,
        _lib.current_stream()))
    return dq, dc, None, None, None, None, None


def _logit_options(dev, sample_weight, candidate_sampling_probability, candidate_ids, score_mask):
  """The device tensors the fused kernels take for the logit options: ``(w, log clip(p), ids, mask)``, None where unset."""
  w = None if sample_weight is None else sample_weight.reshape(-1).to(dev, torch.float32).contiguous()
  corr = None
  if candidate_sampling_probability is not None:                      # loss.py:157-158
    corr = torch.log(torch.clamp(candidate_sampling_probability.to(dev, torch.float32),
                                 1e-6, 1.0)).contiguous()
  ids = None if candidate_ids is None else candidate_ids.reshape(-1).to(dev).long().contiguous()
  mask = None if score_mask is None else score_mask.to(dev).to(torch.uint8).contiguous()
  return w, corr, ids, mask


def _fused_softmax_loss(query_embeddings, candidate_embeddings, sample_weight, temperature,
                        candidate_sampling_probability, candidate_ids, score_mask):
  """Turns the options of the two public functions into the device tensors of the kernels and runs them."""
  inv_t = 1.0 if temperature is None else 1.0 / float(temperature)
  w, corr, ids, mask = _logit_options(query_embeddings.device, sample_weight, candidate_sampling_probability,
                                      candidate_ids, score_mask)
  return _InBatchSoftmaxFn.apply(query_embeddings.to(torch.float32),
                                 candidate_embeddings.to(torch.float32), w, inv_t, corr, ids, mask)


def in_batch_softmax_loss(query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor,
                          sample_weight: Optional[torch.Tensor] = None,
                          temperature: Optional[float] = None,
                          candidate_sampling_probability: Optional[torch.Tensor] = None,
                          candidate_ids: Optional[torch.Tensor] = None,
                          score_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Functional form of the fused default loss (retrieval.py:172-210)."""
  if query_embeddings.dim() != 2:
    raise ValueError(f"queries must be [B, D] (got {tuple(query_embeddings.shape)}).")
  return _fused_softmax_loss(query_embeddings, candidate_embeddings, sample_weight, temperature,
                             candidate_sampling_probability, candidate_ids, score_mask)


MAX_FUSED_HEADS = 32   # head slots of a query share one 32-row MFMA block (csrc/softmax.hip)


def multi_head_in_batch_softmax_loss(query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor,
                                     sample_weight: Optional[torch.Tensor] = None,
                                     temperature: Optional[float] = None,
                                     candidate_sampling_probability: Optional[torch.Tensor] = None,
                                     candidate_ids: Optional[torch.Tensor] = None,
                                     score_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
  """``in_batch_softmax_loss`` for multi-head queries ``[B, H, D]`` (retrieval.py:172-176): the logit of a
  (query, candidate) pair is the max over the query's heads of the dot products, taken before the temperature
  and the other adjustments.  ``H <= 32``, ``D <= 128``; no ``[B * H, C]`` or ``[B, C]`` tensor is built."""
  if query_embeddings.dim() != 3:
    raise ValueError(f"multi-head queries must be [B, H, D] (got {tuple(query_embeddings.shape)}).")
  heads, d = query_embeddings.shape[1], query_embeddings.shape[2]
  if not 1 <= heads <= MAX_FUSED_HEADS:
    raise ValueError(f"multi_head_in_batch_softmax_loss: {heads} heads outside [1, {MAX_FUSED_HEADS}]")
  if d > 128:
    raise ValueError(f"multi_head_in_batch_softmax_loss: embedding dim {d} above 128")
  return _fused_softmax_loss(query_embeddings, candidate_embeddings, sample_weight, temperature,
                             candidate_sampling_probability, candidate_ids, score_mask)


def hard_negative_softmax_loss(query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor,
                               num_hard_negatives: int, sample_weight: Optional[torch.Tensor] = None,
                               temperature: Optional[float] = None) -> torch.Tensor:
  """``HardNegativeMining`` + softmax cross-entropy (layers/loss.py:61-111, tasks/retrieval.py:205-210)
  WITHOUT the ``[B, C]`` logits matrix, for logits that are plain (temperature-scaled) dot products: the
  reference keeps, per row, the positive and the ``num_hard_negatives`` highest negatives
  (``top_k(logits + labels * MAX_FLOAT, k + 1, sorted=False)``); here the fused top-K search of the batch's
  candidates (``top_k_of_block``: exact f32 scores, no matrix) names those rows, the lookup kernel gathers
  them (its backward is the deterministic scatter-add) and the cross-entropy runs on ``[B, k + 1]``
  logits.  Boundary ties between equal negatives pick different but equally scored rows: same loss."""
  from recommenders_amd.layers import embedding as emb_layers
  from recommenders_amd.layers import factorized_top_k as ftk
  q = query_embeddings.to(torch.float32)
  c = candidate_embeddings.to(torch.float32)
  nq, nc = q.shape[0], c.shape[0]
  num_sampled = min(int(num_hard_negatives) + 1, nc)                    # loss.py:91
  n_neg = num_sampled - 1
  pos = (q * c[:nq]).sum(dim=1, keepdim=True)                            # [B, 1]
  if n_neg > 0:
    with torch.no_grad():
      # the positive may or may not be among the best n_neg + 1 rows: search one more and drop it
      _, rows = ftk.top_k_of_block(q.detach(), c.detach(), min(n_neg + 1, nc))
      is_pos = (rows == torch.arange(nq, device=rows.device, dtype=rows.dtype)[:, None])
      order = torch.sort(is_pos.to(torch.int8), dim=1, stable=True).indices[:, :n_neg]   # negatives first, by score
      neg_rows = torch.gather(rows, 1, order).long()
    neg = (emb_layers._GatherFn.apply(c, neg_rows) * q[:, None, :]).sum(dim=2)            # [B, n_neg]
    logits = torch.cat([pos, neg], dim=1)
  else:
    logits = pos
  if temperature is not None:
    logits = logits / float(temperature)                                 # :187-188
  per_row = torch.logsumexp(logits, dim=1) - logits[:, 0]                # CE with the label on column 0
  if sample_weight is not None:
    per_row = per_row * sample_weight.reshape(-1).to(per_row.device, torch.float32)
  return per_row.sum()                                                   # Reduction.SUM (:86-87)


class _MinedSoftmaxFn(torch.autograd.Function):
  """``(loss, tau, cut)`` of the mined in-batch softmax (``tfrs_inbatch_mined_select`` / ``_ce_fwd`` / ``_ce_bwd``):
  the kept set of row ``b`` is its positive and the ``n`` negatives with the largest adjusted logits, written as the
  threshold ``tau[b]`` and the cut column ``cut[b]`` that the metric count reuses.  Only the loss is differentiable."""

  @staticmethod
  def _workspace(lib, q, c):
    return torch.empty((lib.tfrs_inbatch_mined_workspace_bytes(q.shape[0], c.shape[0], q.shape[1]),),
                       dtype=torch.uint8, device=q.device)

  @staticmethod
  def forward(ctx, q, c, sample_weight, temperature, log_corr, cand_ids, score_mask, num_hard_negatives):
    lib = _lib.load()
    q = q.contiguous()
    c = c.contiguous()
    (nq, d), nc = q.shape, c.shape[0]
    ws = _MinedSoftmaxFn._workspace(lib, q, c)
    tau = torch.empty((nq,), dtype=torch.float32, device=q.device)
    cut = torch.empty((nq,), dtype=torch.int64, device=q.device)
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    lse = torch.empty((nq,), dtype=torch.float32, device=q.device)
    pos = torch.empty((nq,), dtype=torch.float32, device=q.device)
    stream = _lib.current_stream()
    _lib.check(lib.tfrs_inbatch_mined_select(
        _lib.ptr(q), _lib.ptr(c), nq, nc, d, float(temperature), _lib.ptr(log_corr), _lib.ptr(cand_ids),
        _lib.ptr(score_mask), int(num_hard_negatives), _lib.ptr(tau), _lib.ptr(cut), _lib.ptr(ws), ws.numel(), stream))
    _lib.check(lib.tfrs_inbatch_mined_ce_fwd(
        _lib.ptr(q), _lib.ptr(c), nq, nc, d, _lib.ptr(sample_weight), float(temperature), _lib.ptr(log_corr),
        _lib.ptr(cand_ids), _lib.ptr(score_mask), _lib.ptr(tau), _lib.ptr(cut), _lib.ptr(loss), _lib.ptr(lse),
        _lib.ptr(pos), _lib.ptr(ws), ws.numel(), stream))
    ctx.save_for_backward(q, c, sample_weight, log_corr, cand_ids, score_mask, tau, cut, lse)
    ctx.temperature = float(temperature)
    ctx.mark_non_differentiable(tau, cut)
    return loss, tau, cut

  @staticmethod
  def backward(ctx, gloss, _gtau, _gcut):
    q, c, sample_weight, log_corr, cand_ids, score_mask, tau, cut, lse = ctx.saved_tensors
    lib = _lib.load()
    dq = torch.empty_like(q)
    dc = torch.empty_like(c)
    g = gloss.to(torch.float32).contiguous()
    ws = _MinedSoftmaxFn._workspace(lib, q, c)
    _lib.check(lib.tfrs_inbatch_mined_ce_bwd(
        _lib.ptr(q), _lib.ptr(c), q.shape[0], c.shape[0], q.shape[1], _lib.ptr(sample_weight), ctx.temperature,
        _lib.ptr(log_corr), _lib.ptr(cand_ids), _lib.ptr(score_mask), _lib.ptr(tau), _lib.ptr(cut), _lib.ptr(lse),
        _lib.ptr(g), _lib.ptr(dq), _lib.ptr(dc), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    return dq, dc, None, None, None, None, None, None


def _mined_softmax(query_embeddings, candidate_embeddings, num_hard_negatives, sample_weight, temperature,
                   candidate_sampling_probability, candidate_ids, score_mask):
  """``(loss, tau, cut)``: see ``mined_in_batch_softmax_loss``."""
  if query_embeddings.dim() != 2:
    raise ValueError(f"queries must be [B, D] (got {tuple(query_embeddings.shape)}).")
  if int(num_hard_negatives) < 0:
    raise ValueError(f"num_hard_negatives must not be negative (got {num_hard_negatives}).")
  w, corr, ids, mask = _logit_options(query_embeddings.device, sample_weight, candidate_sampling_probability,
                                      candidate_ids, score_mask)
  return _MinedSoftmaxFn.apply(query_embeddings.to(torch.float32), candidate_embeddings.to(torch.float32), w,
                               1.0 if temperature is None else float(temperature), corr, ids, mask,
                               int(num_hard_negatives))


def mined_in_batch_softmax_loss(query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor,
                                num_hard_negatives: int, sample_weight: Optional[torch.Tensor] = None,
                                temperature: Optional[float] = None,
                                candidate_sampling_probability: Optional[torch.Tensor] = None,
                                candidate_ids: Optional[torch.Tensor] = None,
                                score_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
  """``HardNegativeMining`` + softmax cross-entropy (layers/loss.py:61-111, tasks/retrieval.py:205-210) over the
  ADJUSTED logits of :178-203 -- temperature (an IEEE division, as the reference's), sampling-probability correction,
  accidental-hit removal (``candidate_ids``), ``score_mask`` -- without the ``[B, C]`` matrix and for any
  ``num_hard_negatives``: an exact radix select on the device finds, per row, the threshold of its
  ``min(num_hard_negatives, C - 1)`` largest negatives (equal values go to the lower column, ``tf.math.top_k``'s
  rule), the loss kernels stream the candidates again and keep what passes it.  ``D <= 128``, ``C >= B``."""
  return _mined_softmax(query_embeddings, candidate_embeddings, num_hard_negatives, sample_weight, temperature,
                        candidate_sampling_probability, candidate_ids, score_mask)[0]


class _CrossReplicaConcatFn(torch.autograd.Function):
  """all-gather along dim 0 with the caller's block first; backward = sum over ranks of the
  gradients of the caller's block (a reduce-scatter)."""

  @staticmethod
  def forward(ctx, values, group):
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    values = values.contiguous()
    n = values.shape[0]
    gathered = torch.empty((world * n,) + tuple(values.shape[1:]), dtype=values.dtype,
                           device=values.device)
    dist.all_gather_into_tensor(gathered, values, group=group)   # blocks in rank order
    ctx.group, ctx.world, ctx.rank = group, world, rank
    return torch.roll(gathered, -rank * n, dims=0)

  @staticmethod
  def backward(ctx, grad):
    import torch.distributed as dist
    world, rank = ctx.world, ctx.rank
    g = torch.roll(grad.reshape((world, -1) + tuple(grad.shape[1:])), rank, dims=0).contiguous()
    out = torch.empty_like(g[0])
    if dist.get_backend(ctx.group) == "gloo":          # gloo has no reduce_scatter
      dist.all_reduce(g, group=ctx.group)
      out.copy_(g[rank])
    else:
      dist.reduce_scatter_tensor(out, g, group=ctx.group)
    return out, None


def cross_replica_concat(values: torch.Tensor, group=None) -> torch.Tensor:
  """``_cross_replica_concat`` of the reference (``tasks/retrieval.py:238-321``) on
  ``torch.distributed``: every rank contributes ``values`` ``[n, ...]`` and receives the
  concatenation of all ranks' blocks ``[world * n, ...]``, rotated so that ITS OWN block comes
  first (rank i sees blocks i, i+1, ..., world-1, 0, ..., i-1) -- so ``labels = eye(n, world*n)``
  still pairs query ``b`` with candidate ``b``.  One RCCL all-gather over xGMI forward; the
  gradient of the caller's block is the sum of every rank's gradient for it (one
  reduce-scatter), i.e. the gradient of the sum of the per-rank losses.  Without an initialised
  process group (or with a single rank) it returns ``values`` unchanged."""
  import torch.distributed as dist
  if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
    return values
  return _CrossReplicaConcatFn.apply(values, group)


class TopKCategoricalAccuracy:
  """``tf.keras.metrics.TopKCategoricalAccuracy(k)`` for ``batch_metrics``: weighted
  mean of ``in_top_k(argmax(labels), logits, k)`` (ties count for the target)."""

  def __init__(self, k: int = 5, name: str = "top_k_categorical_accuracy"):
    self.k = k
    self.name = name
    self._mean = tfrs_metrics.Mean(name)

  def update_state(self, labels, logits, sample_weight=None):
    target = torch.gather(logits, 1, torch.argmax(labels, dim=1, keepdim=True))
    greater = (logits > target).sum(dim=1)
    hit = ((greater < self.k) & torch.isfinite(target.squeeze(1))).to(torch.float32)
    self._mean.update_state(hit, sample_weight)

  def update_from_embeddings(self, q: torch.Tensor, c: torch.Tensor, sample_weight=None) -> None:
    """The same update WITHOUT the ``[B, C]`` logits matrix, for unadjusted logits ``q @ c.T``
    (labels = eye): ``in_top_k`` only asks how many logits of a row are strictly greater than the
    positive's, so the batch's candidates are swept by the rank-count kernel
    (``tfrs_rank_count_accumulate``: f32 MFMA, the d-ordered fma chain -- the positive ties exactly
    with its own column) and ``tfrs_topk_hits_update`` turns the counts into hit indicators."""
    lib = _lib.load()
    nq, d = q.shape
    q = q.detach().to(torch.float32).contiguous()
    c = c.detach().to(torch.float32).contiguous()
    counts = torch.zeros((nq,), dtype=torch.int32, device=q.device)
    _lib.check(lib.tfrs_rank_count_accumulate(
        _lib.ptr(q), _lib.ptr(c), nq, d, _lib.ptr(c), None, 0, c.shape[0], c.shape[0], _lib.ptr(counts), 1,
        _lib.current_stream()))
    self._update_from_counts(counts, sample_weight)

  def update_from_adjusted(self, q: torch.Tensor, c: torch.Tensor, sample_weight=None, temperature=None,
                           candidate_sampling_probability=None, candidate_ids=None, score_mask=None,
                           tau=None, cut=None) -> None:
    """The same update on the ADJUSTED logits the loss saw (:178-208), still without the matrix:
    ``tfrs_inbatch_mined_rank_count`` re-scores the batch with the temperature division, the sampling correction,
    accidental-hit removal and the score mask applied in registers and counts, per row, the kept negatives strictly
    above the positive.  ``tau`` / ``cut``: the kept set of the mined loss (``None``: every column is kept)."""
    lib = _lib.load()
    nq, d = q.shape
    q = q.detach().to(torch.float32).contiguous()
    c = c.detach().to(torch.float32).contiguous()
    _, corr, ids, mask = _logit_options(q.device, None, candidate_sampling_probability, candidate_ids, score_mask)
    counts = torch.empty((nq,), dtype=torch.int32, device=q.device)
    ws = _MinedSoftmaxFn._workspace(lib, q, c)
    _lib.check(lib.tfrs_inbatch_mined_rank_count(
        _lib.ptr(q), _lib.ptr(c), nq, c.shape[0], d, 1.0 if temperature is None else float(temperature),
        _lib.ptr(corr), _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(tau), _lib.ptr(cut), _lib.ptr(counts), _lib.ptr(ws),
        ws.numel(), _lib.current_stream()))
    self._update_from_counts(counts, sample_weight)

  def _update_from_counts(self, counts: torch.Tensor, sample_weight) -> None:
    """The tail of both matrix-free updates: per-row rank counts (bit 31: a non-finite positive) become hit
    indicators (``tfrs_topk_hits_update``) and enter the weighted mean."""
    import ctypes
    nq = counts.shape[0]
    hits = torch.empty((1, nq), dtype=torch.float32, device=counts.device)
    scratch = torch.zeros((3,), dtype=torch.float32, device=counts.device)     # state[2], result[1] (unused)
    ks = (ctypes.c_int32 * 1)(int(self.k))
    _lib.check(_lib.load().tfrs_topk_hits_update(_lib.ptr(counts), nq, ks, 1, None, _lib.ptr(scratch),
                                                 _lib.ptr(scratch[2:]), _lib.ptr(hits), _lib.current_stream()))
    self._mean.update_state(hits[0], sample_weight)

  def result(self):
    return self._mean.result()

  def reset_states(self):
    self._mean.reset_states()


class _LogitsCeFn(torch.autograd.Function):
  """``sum_i w_i * (-sum_j y_ij log_softmax(S_i)_j)`` on an explicit ``[B, C]`` logits matrix
  (``tfrs_logits_ce_fwd`` / ``_bwd``): Keras ``CategoricalCrossentropy(from_logits=True, reduction=SUM)``
  (reference ``tasks/retrieval.py:86-87``) for the paths that have to build the matrix."""

  @staticmethod
  def forward(ctx, scores, labels, sample_weight):
    scores = scores.contiguous().to(torch.float32)
    labels = labels.contiguous().to(torch.float32)
    nq, nc = scores.shape
    w = None
    if sample_weight is not None:
      # one weight per row; a scalar / one-element weight broadcasts as in Keras -- anything else is an error here,
      # not an out-of-bounds read in the kernel
      w = torch.as_tensor(sample_weight).reshape(-1).to(scores.device, torch.float32)
      if w.numel() == 1:
        w = w.expand(nq)
      elif w.numel() != nq:
        raise ValueError(f"sample_weight has {w.numel()} elements for {nq} rows of logits")
      w = w.contiguous()
    rows = torch.empty((3, max(nq, 1)), dtype=torch.float32, device=scores.device)   # row loss, lse, sum of labels
    _lib.check(_lib.load().tfrs_logits_ce_fwd(_lib.ptr(scores), _lib.ptr(labels), nq, nc, _lib.ptr(w),
                                              _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(rows[2]),
                                              _lib.current_stream()))
    ctx.save_for_backward(scores, labels, rows)
    ctx.weight = w
    return rows[0, :nq].sum()

  @staticmethod
  def backward(ctx, grad):
    scores, labels, rows = ctx.saved_tensors
    nq, nc = scores.shape
    ds = torch.empty_like(scores)
    g = grad.reshape(1).to(torch.float32).contiguous()
    _lib.check(_lib.load().tfrs_logits_ce_bwd(_lib.ptr(scores), _lib.ptr(labels), nq, nc, _lib.ptr(ctx.weight),
                                              _lib.ptr(rows[1]), _lib.ptr(rows[2]), _lib.ptr(g), _lib.ptr(ds),
                                              _lib.current_stream()))
    return ds, None, None


def logits_softmax_ce_sum(scores: torch.Tensor, labels: torch.Tensor,
                          sample_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
  return _LogitsCeFn.apply(scores, labels, sample_weight)


class LossRoute(enum.Enum):
  """How ``Retrieval.forward`` computes the loss."""
  FUSED_2D = "fused 2-D"                        # in_batch_softmax_loss
  FUSED_MULTI_HEAD = "fused multi-head"         # multi_head_in_batch_softmax_loss
  TOPK_HARD_NEGATIVES = "top-K hard negatives"  # hard_negative_softmax_loss: plain dot products, the top-K search
  MINED = "mined"                               # mined_in_batch_softmax_loss: radix select + keep predicate
  MATRIX_CE = "matrix cross-entropy"            # the built-in loss on the explicit [B, C] logits
  CUSTOM = "custom loss"                        # a user-supplied loss: its contract IS the matrix


class MetricRoute(enum.Enum):
  """How ``Retrieval.forward`` updates ``batch_metrics``."""
  NONE = "none"
  PLAIN_COUNT = "rank count on plain dot products"    # TopKCategoricalAccuracy.update_from_embeddings
  ADJUSTED_COUNT = "rank count on adjusted logits"    # ... .update_from_adjusted (the mined kept set included)
  MATRIX = "matrix"                                   # update_state on the explicit [B, C] logits


def pick_routes(*, custom_loss: bool, query_rank: int, dim: int, heads: int, nq: int, nc: int,
                num_hard_negatives: Optional[int], temperature: bool, sampling_correction: bool,
                accidental_hits: bool, score_mask: bool, batch_metric_classes: Sequence[type], explicit: bool):
  """``(LossRoute, MetricRoute)`` of one ``Retrieval.forward`` call, from the facts of its configuration alone:
  whether a user loss is set, the queries' rank / embedding dim / heads (rank 3), the row counts,
  ``num_hard_negatives``, which logit options are set, the classes of the batch metrics that will be updated (empty: none) and the
  ``TFRS_RETRIEVAL_EXPLICIT=1`` switch.  The explicit ``[B, C]`` matrix is built exactly when one of the two routes
  uses it (``needs_matrix``).  The fused kernels hold an embedding row in registers: dims above 128 take the matrix
  (the reference accepts any dim).  A 2-D built-in loss without hard negatives is FUSED_2D whatever the row counts:
  with more queries than candidates the C entry reports the error."""
  has_metrics = len(batch_metric_classes) > 0
  foreign_metrics = any(cls is not TopKCategoricalAccuracy for cls in batch_metric_classes)
  options = sampling_correction or accidental_hits or score_mask     # what makes a logit more than a scaled dot product
  mined_ok = not explicit and nc >= nq                               # the envelope of the tfrs_inbatch_mined_* entries

  if custom_loss:
    loss = LossRoute.CUSTOM
  elif query_rank != 2:
    fused = (query_rank == 3 and num_hard_negatives is None and dim <= 128 and 1 <= heads <= MAX_FUSED_HEADS
             and not has_metrics)
    loss = LossRoute.FUSED_MULTI_HEAD if fused else LossRoute.MATRIX_CE
  elif dim > 128:
    loss = LossRoute.MATRIX_CE
  elif num_hard_negatives is None:
    loss = LossRoute.FUSED_2D
  elif not options and int(num_hard_negatives) + 2 <= 1024 and not has_metrics:
    loss = LossRoute.TOPK_HARD_NEGATIVES
  elif mined_ok and not foreign_metrics:        # a foreign batch metric needs the matrix anyway
    loss = LossRoute.MINED
  else:
    loss = LossRoute.MATRIX_CE

  if not has_metrics:
    metric = MetricRoute.NONE
  elif foreign_metrics:
    metric = MetricRoute.MATRIX
  elif loss is LossRoute.FUSED_2D and not temperature and not options:
    metric = MetricRoute.PLAIN_COUNT
  elif loss is LossRoute.MINED or (loss is LossRoute.FUSED_2D and mined_ok):
    metric = MetricRoute.ADJUSTED_COUNT         # the temperature divides there as in the reference
  else:
    metric = MetricRoute.MATRIX
  return loss, metric


def needs_matrix(loss_route: LossRoute, metric_route: MetricRoute) -> bool:
  return loss_route in (LossRoute.MATRIX_CE, LossRoute.CUSTOM) or metric_route is MetricRoute.MATRIX


class Retrieval(torch.nn.Module, base.Task):
  """A factorized retrieval task (reference :29-235)."""

  def __init__(self, loss: Optional[Callable] = None,
               metrics: Optional[Union[Sequence[tfrs_metrics.Factorized],
                                       tfrs_metrics.Factorized]] = None,
               batch_metrics: Optional[List] = None, loss_metrics: Optional[List] = None,
               temperature: Optional[float] = None, num_hard_negatives: Optional[int] = None,
               remove_accidental_hits: bool = False, name: Optional[str] = None,
               cross_replica_negatives: bool = False, process_group=None) -> None:
    """``cross_replica_negatives`` (not in the reference's signature, which defines
    ``_cross_replica_concat`` :238-321 but never calls it): under ``torch.distributed`` every
    rank scores its queries against the candidates of ALL ranks -- ``world`` times more
    in-batch negatives for one all-gather of ``[B, D]`` per rank.  Candidate ids and
    sampling probabilities are gathered the same way; a ``score_mask`` must already have the
    gathered width."""
    super().__init__()
    self._cross_replica_negatives = cross_replica_negatives
    self._process_group = process_group
    self.name = name or "retrieval"
    self._loss = loss            # None -> fused in-batch softmax (:86-87)
    if metrics is None:
      metrics = []
    if not isinstance(metrics, Sequence):
      metrics = [metrics]
    self._factorized_metrics = list(metrics)
    self._batch_metrics = batch_metrics or []
    self._loss_metrics = loss_metrics or []
    self._temperature = temperature
    self._num_hard_negatives = num_hard_negatives
    self._remove_accidental_hits = remove_accidental_hits

  @property
  def factorized_metrics(self):
    return self._factorized_metrics                                     # :101-106

  @factorized_metrics.setter
  def factorized_metrics(self, value) -> None:                          # :108-119
    if not isinstance(value, Sequence):
      value = []                  # (the reference's behaviour: a bare metric object clears the list)
    self._factorized_metrics = list(value)

  def __setattr__(self, name, value):
    # torch.nn.Module.__setattr__ registers a Module VALUE as a sub-module before any property setter is
    # consulted: `task.factorized_metrics = FactorizedTopK(...)` would add a child named like the property
    # and leave the list the task updates untouched.  Route the name to the setter, as Keras does.
    if name == "factorized_metrics":
      type(self).factorized_metrics.fset(self, value)
      return
    super().__setattr__(name, value)

  @property
  def metrics(self):
    """All metric objects, like Keras' ``layer.metrics``."""
    out = []
    for m in self._factorized_metrics:
      out.extend(m.metrics)
    return out + list(self._batch_metrics) + list(self._loss_metrics)

  def _logits_and_labels(self, q, c, candidate_sampling_probability, candidate_ids,
                         score_mask):
    """Explicit logits following :172-208 (only for paths that need the matrix)."""
    if q.dim() == 3:                                                    # :172-176 maxsim
      nq, heads, d = q.shape
      flat = _DenseFn.apply(q.reshape(nq * heads, d).contiguous(), c.t().contiguous(), None)
      scores = flat.reshape(nq, heads, -1).max(dim=1).values
    else:
      scores = _DenseFn.apply(q.contiguous(), c.t().contiguous(), None)  # :178-180
    nq, nc = scores.shape
    labels = torch.eye(nq, nc, dtype=torch.float32, device=scores.device)   # :185
    if self._temperature is not None:
      scores = scores / self._temperature                               # :187-188
    if candidate_sampling_probability is not None:
      scores = loss_layers.SamplingProbablityCorrection()(
          scores, candidate_sampling_probability.to(scores.device))     # :190-192
    if self._remove_accidental_hits:
      scores = loss_layers.RemoveAccidentalHits()(labels, scores,
                                                  candidate_ids.to(scores.device))  # :200
    if score_mask is not None:
      scores = torch.where(score_mask.to(scores.device).bool(), scores,
                           torch.full_like(scores, MIN_FLOAT))          # :202-203
    if self._num_hard_negatives is not None:
      scores, labels = loss_layers.HardNegativeMining(self._num_hard_negatives)(
          scores, labels)                                               # :205-208
    return scores, labels

  def forward(self, query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor,
              sample_weight: Optional[torch.Tensor] = None,
              candidate_sampling_probability: Optional[torch.Tensor] = None,
              candidate_ids: Optional[torch.Tensor] = None, compute_metrics: bool = True,
              compute_batch_metrics: bool = True,
              score_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    if self._remove_accidental_hits and candidate_ids is None:          # :194-199
      raise ValueError("When accidental hit removal is enabled, candidate ids "
                       "must be supplied.")
    q, c = query_embeddings, candidate_embeddings
    if self._cross_replica_negatives:
      c = cross_replica_concat(c, self._process_group)
      if candidate_ids is not None:
        candidate_ids = cross_replica_concat(torch.as_tensor(candidate_ids).to(c.device),
                                             self._process_group)
      if candidate_sampling_probability is not None:
        candidate_sampling_probability = cross_replica_concat(
            torch.as_tensor(candidate_sampling_probability).to(c.device), self._process_group)
    if sample_weight is not None and not isinstance(sample_weight, torch.Tensor):
      sample_weight = torch.as_tensor(np.asarray(sample_weight, dtype=np.float32))
    if sample_weight is not None:
      sample_weight = sample_weight.to(q.device)

    # (captured step: the metric branch below forks HERE, in front of the loss kernels -- _streams.mark)
    fork_point = (_streams.mark(q.device) if compute_metrics and q.dim() == 2 and self._factorized_metrics else None)

    # TFRS_RETRIEVAL_EXPLICIT=1 (read per call: tests and tools/bench_hard_negatives.py switch it) keeps hard
    # negatives / batch metrics over adjusted logits on the explicit [B, C] matrix, the comparator of the mined route
    loss_route, metric_route = pick_routes(
        custom_loss=self._loss is not None, query_rank=q.dim(), dim=q.shape[-1],
        heads=q.shape[1] if q.dim() == 3 else 1, nq=q.shape[0], nc=c.shape[0],
        num_hard_negatives=self._num_hard_negatives, temperature=self._temperature is not None,
        sampling_correction=candidate_sampling_probability is not None,
        accidental_hits=self._remove_accidental_hits, score_mask=score_mask is not None,
        batch_metric_classes=[type(m) for m in self._batch_metrics] if compute_batch_metrics else [],
        explicit=os.environ.get("TFRS_RETRIEVAL_EXPLICIT") == "1")
    scores = labels = None
    if needs_matrix(loss_route, metric_route):
      scores, labels = self._logits_and_labels(
          q, c, candidate_sampling_probability, candidate_ids, score_mask)

    accidental_ids = candidate_ids if self._remove_accidental_hits else None
    tau = cut = None
    if loss_route is LossRoute.FUSED_2D:
      loss = in_batch_softmax_loss(                                     # fused :172-210
          q, c, sample_weight, self._temperature, candidate_sampling_probability, accidental_ids, score_mask)
    elif loss_route is LossRoute.FUSED_MULTI_HEAD:
      loss = multi_head_in_batch_softmax_loss(                          # fused :172-176, :185-210
          q, c, sample_weight, self._temperature, candidate_sampling_probability, accidental_ids, score_mask)
    elif loss_route is LossRoute.TOPK_HARD_NEGATIVES:
      loss = hard_negative_softmax_loss(q, c, self._num_hard_negatives, sample_weight, self._temperature)
    elif loss_route is LossRoute.MINED:
      loss, tau, cut = _mined_softmax(                                  # fused :178-210 with :205-208
          q, c, self._num_hard_negatives, sample_weight, self._temperature, candidate_sampling_probability,
          accidental_ids, score_mask)
    elif loss_route is LossRoute.MATRIX_CE:
      # CategoricalCrossentropy(from_logits, SUM) on the explicit logits (:86-87, :210): row-wise HIP kernels
      loss = logits_softmax_ce_sum(scores, labels, sample_weight)
    else:
      loss = self._loss(y_true=labels, y_pred=scores, sample_weight=sample_weight)

    for metric in self._loss_metrics:                                   # :213-214
      metric.update_state(loss.detach())

    if compute_metrics and q.dim() == 2:                                # :216-226
      # (a parallel branch of a captured step: the update needs the embeddings only, not the loss -- _streams.py)
      with torch.no_grad(), _streams.forked(q.device, after=fork_point):
        for metric in self._factorized_metrics:
          metric.update_state(q.detach(), c.detach()[:q.shape[0]],
                              true_candidate_ids=candidate_ids, sample_weight=sample_weight)

    if compute_batch_metrics:                                           # :228-232
      with torch.no_grad():
        for metric in self._batch_metrics:
          if metric_route is MetricRoute.PLAIN_COUNT:
            metric.update_from_embeddings(q, c, sample_weight=sample_weight)
          elif metric_route is MetricRoute.ADJUSTED_COUNT:
            metric.update_from_adjusted(q, c, sample_weight, self._temperature, candidate_sampling_probability,
                                        accidental_ids, score_mask, tau, cut)
          else:
            metric.update_state(labels, scores.detach(), sample_weight=sample_weight)

    return loss

  call = forward
