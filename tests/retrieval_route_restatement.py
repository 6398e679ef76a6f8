"""Restatement of the route choice of ``Retrieval.forward`` as it stood BEFORE ``pick_routes`` (test infrastructure
only): the nine interlocking booleans, the hand-written ``need_matrix`` formula and the ``if / elif`` chains, copied
verbatim from that ``forward`` and wrapped as a function of the configuration facts they read.  The stand-ins
(``self``, ``q``, ``c``, ``os`` ...) carry exactly the attributes the block touches.  It exists so that
``tests/test_retrieval_route_host.py`` can compare ``pick_routes`` against it on every combination; do not simplify
it.
"""

import types

MAX_FUSED_HEADS = 32


class _Tensor:
  """``dim()`` and ``shape`` of an embedding tensor."""

  def __init__(self, *shape):
    self.shape = tuple(shape)

  def dim(self):
    return len(self.shape)


def routes(*, custom_loss, query_rank, dim, heads, nq, nc, num_hard_negatives, temperature, sampling_correction,
           accidental_hits, score_mask, batch_metrics, counted_class, explicit, compute_batch_metrics=True):
  """``(loss route, metric route, need_matrix)`` as the old block chose them; the routes by the names of
  ``LossRoute`` / ``MetricRoute`` members.  ``batch_metrics``: metric OBJECTS; ``counted_class``: the class the block
  calls ``TopKCategoricalAccuracy``."""
  TopKCategoricalAccuracy = counted_class
  self = types.SimpleNamespace(
      _loss=(lambda **kw: None) if custom_loss else None, _temperature=0.5 if temperature else None,
      _num_hard_negatives=num_hard_negatives, _remove_accidental_hits=accidental_hits,
      _batch_metrics=list(batch_metrics))
  q = _Tensor(nq, heads, dim) if query_rank == 3 else _Tensor(nq, dim)
  c = _Tensor(nc, dim)
  candidate_sampling_probability = object() if sampling_correction else None
  score_mask = object() if score_mask else None
  os = types.SimpleNamespace(environ={"TFRS_RETRIEVAL_EXPLICIT": "1"} if explicit else {})

  # ---- verbatim from Retrieval.forward ----
  # the fused kernels hold an embedding row in registers: dims above 128 (outside their
  # envelope; the reference accepts any dim) take the explicit-logits path below
  wide = q.dim() == 2 and q.shape[-1] > 128
  has_batch_metrics = compute_batch_metrics and len(self._batch_metrics) > 0
  adjusted = (self._temperature is not None or candidate_sampling_probability is not None
              or self._remove_accidental_hits or score_mask is not None)
  # TFRS_RETRIEVAL_EXPLICIT=1 (read per call: tests and tools/bench_hard_negatives.py switch it) keeps hard
  # negatives / batch metrics over adjusted logits on the explicit [B, C] matrix, the comparator of the mined route
  mined_ok = (os.environ.get("TFRS_RETRIEVAL_EXPLICIT") != "1" and self._loss is None and q.dim() == 2
              and not wide and c.shape[0] >= q.shape[0])
  counted_metrics = has_batch_metrics and all(type(m) is TopKCategoricalAccuracy for m in self._batch_metrics)
  # batch metrics of unadjusted logits need a rank count per row, not the matrix (missing item 3 of
  # round 3's review): tfrs_rank_count_accumulate on the plain dot products
  fused_batch_metrics = (
      counted_metrics and q.dim() == 2 and not wide and self._loss is None
      and self._num_hard_negatives is None and not adjusted)
  # hard-negative mining over plain (temperature-scaled) dot products: the top-K search names the rows
  fused_hard_negatives = (
      self._num_hard_negatives is not None and self._loss is None and q.dim() == 2 and not wide
      and candidate_sampling_probability is None and not self._remove_accidental_hits
      and score_mask is None and int(self._num_hard_negatives) + 2 <= 1024
      and not has_batch_metrics)
  # every other hard-negative configuration of the built-in loss: the radix select and the keep predicate inside
  # the streaming kernels (mined_in_batch_softmax_loss) -- unless a foreign batch metric needs the matrix anyway
  mined_hard_negatives = (
      self._num_hard_negatives is not None and not fused_hard_negatives and mined_ok
      and (counted_metrics or not has_batch_metrics))
  # ... and batch metrics of ADJUSTED (or mined) logits: the rank count over the same logit function; the
  # temperature divides there as in the reference, so near-ties merge as they do on the matrix
  adjusted_batch_metrics = (
      counted_metrics and not fused_batch_metrics and mined_ok
      and (self._num_hard_negatives is None or mined_hard_negatives))
  # multi-head queries: the fused max-sim kernels under the conditions of the 2-D fused route
  fused_multi_head = (
      q.dim() == 3 and self._loss is None and self._num_hard_negatives is None
      and q.shape[-1] <= 128 and 1 <= q.shape[1] <= MAX_FUSED_HEADS
      and not has_batch_metrics)
  need_matrix = ((q.dim() == 3 and not fused_multi_head) or self._loss is not None
                 or (self._num_hard_negatives is not None and not fused_hard_negatives
                     and not mined_hard_negatives) or wide
                 or (has_batch_metrics and not fused_batch_metrics and not adjusted_batch_metrics))

  if self._loss is None and q.dim() == 2 and self._num_hard_negatives is None and not wide:
    loss = "FUSED_2D"                         # in_batch_softmax_loss
  elif fused_multi_head:
    loss = "FUSED_MULTI_HEAD"                 # multi_head_in_batch_softmax_loss
  elif fused_hard_negatives:
    loss = "TOPK_HARD_NEGATIVES"              # hard_negative_softmax_loss
  elif mined_hard_negatives:
    loss = "MINED"                            # _mined_softmax
  elif self._loss is None:
    loss = "MATRIX_CE"                        # logits_softmax_ce_sum(scores, labels, sample_weight)
  else:
    loss = "CUSTOM"                           # self._loss(y_true=labels, y_pred=scores, ...)

  metric = "NONE"
  if compute_batch_metrics:
    for _ in self._batch_metrics:
      if fused_batch_metrics:
        metric = "PLAIN_COUNT"                # metric.update_from_embeddings
      elif adjusted_batch_metrics:
        metric = "ADJUSTED_COUNT"             # metric.update_from_adjusted
      else:
        metric = "MATRIX"                     # metric.update_state(labels, scores.detach(), ...)
  # ---- end of the verbatim block ----
  return loss, metric, bool(need_matrix)
