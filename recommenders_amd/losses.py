"""Keras losses the ranking task uses (tf.keras.losses semantics, restated).

``BinaryCrossentropy(from_logits=False)``: probabilities are clipped to
``[1e-7, 1 - 1e-7]``, the per-sample loss is the mean over the last axis of
``-(y log p + (1 - y) log(1 - p))``; ``reduction``: ``"sum_over_batch_size"`` (Keras AUTO:
weighted sum / number of samples), ``"sum"`` or ``"none"`` (per-sample vector, as
``experimental/models/ranking.py:116-118`` asks for).  ``MeanSquaredError`` likewise.
"""

from typing import Optional

import torch

_EPS = 1e-7


class _Loss:
  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = None):
    if reduction in ("auto", "AUTO"):
      reduction = "sum_over_batch_size"
    if reduction not in ("sum_over_batch_size", "sum", "none"):
      raise ValueError(f"Unknown reduction: {reduction!r}")
    self.reduction = reduction
    self.name = name

  def _per_sample(self, y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    raise NotImplementedError

  def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
    y_pred = y_pred.to(torch.float32)
    y_true = y_true.to(y_pred.device, torch.float32).reshape(y_pred.shape)
    per = self._per_sample(y_true, y_pred)                      # [batch, ...] last axis reduced
    if sample_weight is not None:
      w = sample_weight.to(per.device, torch.float32)
      if w.dim() == per.dim() + 1 and w.shape[-1] == 1:        # Keras squeezes a trailing 1
        w = w.squeeze(-1)
      per = per * w
    if self.reduction == "none":
      return per
    if self.reduction == "sum":
      return per.sum()
    return per.sum() / per.numel()


class BinaryCrossentropy(_Loss):
  def __init__(self, from_logits: bool = False, reduction: str = "sum_over_batch_size",
               name: Optional[str] = "binary_crossentropy"):
    super().__init__(reduction, name)
    self.from_logits = from_logits

  def _per_sample(self, y_true, y_pred):
    if self.from_logits:
      bce = torch.nn.functional.binary_cross_entropy_with_logits(y_pred, y_true, reduction="none")
    else:
      p = torch.clamp(y_pred, _EPS, 1.0 - _EPS)
      bce = -(y_true * torch.log(p) + (1.0 - y_true) * torch.log(1.0 - p))
    return bce.mean(dim=-1) if bce.dim() > 1 else bce


class MeanSquaredError(_Loss):
  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "mean_squared_error"):
    super().__init__(reduction, name)

  def _per_sample(self, y_true, y_pred):
    se = (y_pred - y_true) ** 2
    return se.mean(dim=-1) if se.dim() > 1 else se


# ------------------------------------------------------------------------------------------------
# Listwise ranking losses: y_true / y_pred are [batch, list]; a position is valid iff
# y_true >= 0 (-1 pads, TF-Ranking's convention).  One fused HIP kernel per direction
# (csrc/listwise.hip): a list lives in LDS and registers, no [B, L, L] tensor exists, the backward
# recomputes from the two inputs.  sample_weight is PER LIST ([B] or [B, 1]).  The two pairwise losses take
# lambda_weight= (DCGLambdaWeight / NDCGLambdaWeight): separate kernels of the same file.
# ------------------------------------------------------------------------------------------------
MAX_LIST_LEN = 1024
_SOFTMAX, _PAIRWISE_LOGISTIC, _PAIRWISE_HINGE, _LIST_MLE = 0, 1, 2, 3


def _listwise_inputs(y_true: torch.Tensor, y_pred: torch.Tensor, what: str, sample_weight=None):
  """float32, contiguous, rank 2, on the GPU, inside the kernels' envelope; every shape is checked before the device."""
  if not isinstance(y_pred, torch.Tensor) or not isinstance(y_true, torch.Tensor):
    raise ValueError(f"{what}: y_true and y_pred must be tensors")
  if y_pred.dim() != 2 or y_true.dim() != 2 or y_true.shape != y_pred.shape:
    raise ValueError(f"{what}: y_true and y_pred must both be [batch, list], got {tuple(y_true.shape)} and "
                     f"{tuple(y_pred.shape)}")
  b, l = y_pred.shape
  if not 1 <= l <= MAX_LIST_LEN:
    raise ValueError(f"{what}: list length {l} outside 1 .. MAX_LIST_LEN = {MAX_LIST_LEN}")
  if b * l >= 2 ** 31:
    raise ValueError(f"{what}: batch * list length = {b * l} must stay below 2^31")
  if sample_weight is not None and tuple(torch.as_tensor(sample_weight).shape) not in ((b,), (b, 1)):
    raise ValueError(f"{what}: sample_weight is per list, [{b}] or [{b}, 1]; got "
                     f"{tuple(torch.as_tensor(sample_weight).shape)}")
  if not y_pred.is_cuda:
    raise RuntimeError(f"{what} needs its inputs on the GPU (device={y_pred.device}); there is no CPU fallback")
  y_pred = y_pred.to(torch.float32).contiguous()
  y_true = y_true.to(y_pred.device, torch.float32).contiguous()
  return y_true, y_pred


class _ListwiseFn(torch.autograd.Function):
  """Per-list loss ``[B]`` of one kind over ``tfrs_listwise_loss_fwd`` / ``_bwd``; only the two inputs are kept."""

  @staticmethod
  def forward(ctx, y_pred, y_true, kind):
    from recommenders_amd import _lib
    b, l = y_pred.shape
    loss = torch.empty((b,), dtype=torch.float32, device=y_pred.device)
    _lib.check(_lib.load().tfrs_listwise_loss_fwd(kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l, _lib.ptr(loss),
                                                   _lib.current_stream()))
    ctx.save_for_backward(y_true, y_pred)
    ctx.kind = kind
    return loss

  @staticmethod
  def backward(ctx, grad):
    from recommenders_amd import _lib
    y_true, y_pred = ctx.saved_tensors
    b, l = y_pred.shape
    scale = grad.to(torch.float32).contiguous()      # [B]: upstream gradient x list weight x reduction factor
    ds = torch.empty_like(y_pred)
    _lib.check(_lib.load().tfrs_listwise_loss_bwd(ctx.kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l,
                                                   _lib.ptr(scale), _lib.ptr(ds), _lib.current_stream()))
    return ds, None, None


class DCGLambdaWeight:
  """LambdaRank / LambdaLoss pair weights on the DCG gain, for ``PairwiseLogisticLoss`` / ``PairwiseHingeLoss``
  (``lambda_weight=``).  With ``r`` the rank of a valid item by score (descending, ties by position
  ascending), ``D0(r) = 1 / log2(r + 1)``, ``D(r) = D0(r)`` up to rank ``topn`` and 0 beyond it, ``G = 2^y - 1`` (divided
  by the list's ideal DCG@topn when ``normalized``; every weight of a list whose ideal DCG is not positive is 0) and
  ``d = |r_i - r_j|``, the term of the pair ``(i, j)`` is multiplied by

      ``w_ij = |G_i - G_j| ((1 - smooth_fraction) |D(r_i) - D(r_j)| + smooth_fraction |D0(d) - D0(d + 1)|)``

  and by 0 when both ranks lie beyond ``topn``.  ``smooth_fraction = 0`` is LambdaRank (``w_ij`` = the change of the
  metric when the two items swap ranks), a positive one LambdaLoss.  The weights are constants of the backward pass.
  Labels must keep ``2^y`` finite in float32 (``y < 128``), as for ``NDCGMetric``."""

  def __init__(self, topn: Optional[int] = None, normalized: bool = False, smooth_fraction: float = 0.0):
    name = type(self).__name__
    try:
      ok = topn is None or (not isinstance(topn, bool) and int(topn) == topn and topn >= 1)
    except (TypeError, ValueError, OverflowError):
      ok = False
    if not ok:
      raise ValueError(f"{name}: topn must be a positive integer or None, got {topn!r}")
    try:
      ok = not isinstance(smooth_fraction, bool) and 0.0 <= float(smooth_fraction) <= 1.0      # (NaN fails both)
    except (TypeError, ValueError):
      ok = False
    if not ok:
      raise ValueError(f"{name}: smooth_fraction must lie in [0, 1], got {smooth_fraction!r}")
    self.topn = None if topn is None else int(topn)
    self.normalized = bool(normalized)
    self.smooth_fraction = float(smooth_fraction)


class NDCGLambdaWeight(DCGLambdaWeight):
  """``DCGLambdaWeight`` normalised by the list's ideal DCG: the pair weights of the NDCG metric."""

  def __init__(self, topn: Optional[int] = None, smooth_fraction: float = 0.0):
    super().__init__(topn=topn, normalized=True, smooth_fraction=smooth_fraction)


class _ListwiseLambdaFn(torch.autograd.Function):
  """``_ListwiseFn`` for a pairwise kind with lambda weights, over ``tfrs_listwise_lambda_fwd`` / ``_bwd``: the backward
  recomputes ranks and weights from the two inputs, nothing else is kept."""

  @staticmethod
  def forward(ctx, y_pred, y_true, kind, topn, normalized, smooth_fraction):
    from recommenders_amd import _lib
    b, l = y_pred.shape
    loss = torch.empty((b,), dtype=torch.float32, device=y_pred.device)
    _lib.check(_lib.load().tfrs_listwise_lambda_fwd(kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l, topn, normalized,
                                                     smooth_fraction, _lib.ptr(loss), _lib.current_stream()))
    ctx.save_for_backward(y_true, y_pred)
    ctx.args = (kind, topn, normalized, smooth_fraction)
    return loss

  @staticmethod
  def backward(ctx, grad):
    from recommenders_amd import _lib
    y_true, y_pred = ctx.saved_tensors
    kind, topn, normalized, smooth_fraction = ctx.args
    b, l = y_pred.shape
    scale = grad.to(torch.float32).contiguous()
    ds = torch.empty_like(y_pred)
    _lib.check(_lib.load().tfrs_listwise_lambda_bwd(kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l, topn, normalized,
                                                     smooth_fraction, _lib.ptr(scale), _lib.ptr(ds),
                                                     _lib.current_stream()))
    return ds, None, None, None, None, None


class _ListwiseLoss(_Loss):
  _KIND = None
  lambda_weight = None

  def _set_lambda_weight(self, lambda_weight):
    if lambda_weight is not None and not isinstance(lambda_weight, DCGLambdaWeight):
      raise ValueError(f"{type(self).__name__}: lambda_weight must be a DCGLambdaWeight, an NDCGLambdaWeight or None, "
                       f"got {lambda_weight!r}")
    self.lambda_weight = lambda_weight

  def _per_sample(self, y_true, y_pred):
    lw = self.lambda_weight
    if lw is None:
      return _ListwiseFn.apply(y_pred, y_true, self._KIND)
    topn = 0 if lw.topn is None else min(lw.topn, 2 ** 31 - 1)
    return _ListwiseLambdaFn.apply(y_pred, y_true, self._KIND, topn, int(lw.normalized), lw.smooth_fraction)

  def __call__(self, y_true, y_pred, sample_weight=None) -> torch.Tensor:
    y_true, y_pred = _listwise_inputs(y_true, y_pred, type(self).__name__, sample_weight)
    if y_pred.shape[0] == 0:                         # no launch: an empty vector, or a zero that still back-propagates
      return y_pred.sum(dim=-1) if self.reduction == "none" else y_pred.sum()
    if sample_weight is not None:
      sample_weight = torch.as_tensor(sample_weight)
    return super().__call__(y_true, y_pred, sample_weight)


class SoftmaxLoss(_ListwiseLoss):
  """``sum_i y_i (logsumexp(s) - s_i)`` over the valid items of a list."""
  _KIND = _SOFTMAX

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "softmax_loss"):
    super().__init__(reduction, name)


class PairwiseLogisticLoss(_ListwiseLoss):
  """``sum_{y_i > y_j} w_ij log(1 + exp(-(s_i - s_j)))`` over the valid pairs of a list; ``w_ij = 1``, or the pair
  weights of ``lambda_weight`` (a ``DCGLambdaWeight`` / ``NDCGLambdaWeight``: LambdaRank, LambdaLoss)."""
  _KIND = _PAIRWISE_LOGISTIC

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "pairwise_logistic_loss",
               lambda_weight: Optional[DCGLambdaWeight] = None):
    super().__init__(reduction, name)
    self._set_lambda_weight(lambda_weight)


class PairwiseHingeLoss(_ListwiseLoss):
  """``sum_{y_i > y_j} w_ij max(0, 1 - (s_i - s_j))`` over the valid pairs of a list; ``w_ij`` as for
  ``PairwiseLogisticLoss``."""
  _KIND = _PAIRWISE_HINGE

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "pairwise_hinge_loss",
               lambda_weight: Optional[DCGLambdaWeight] = None):
    super().__init__(reduction, name)
    self._set_lambda_weight(lambda_weight)


class ListMLELoss(_ListwiseLoss):
  """Negative Plackett-Luce log-likelihood of the label order (label descending, ties by position ascending:
  deterministic, where TF-Ranking shuffles ties)."""
  _KIND = _LIST_MLE

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "list_mle_loss"):
    super().__init__(reduction, name)


# ------------------------------------------------------------------------------------------------
# Pair-sum losses: every item first needs a sum over the other items of its list (a soft rank, a
# restricted logsumexp) and the gradient is a second pair sum over those; one fused kernel per direction
# (csrc/listwise.hip: listwise_pairsum_kernel), no [B, L, L] tensor, the backward recomputes from the two inputs.
# ------------------------------------------------------------------------------------------------
_APPROX_NDCG, _APPROX_MRR, _UNIQUE_SOFTMAX = 0, 1, 2


class _PairSumFn(torch.autograd.Function):
  """Per-list loss ``[B]`` of one pair-sum kind over ``tfrs_listwise_pairsum_fwd`` / ``_bwd``; only the two inputs are
  kept."""

  @staticmethod
  def forward(ctx, y_pred, y_true, kind, temperature):
    from recommenders_amd import _lib
    b, l = y_pred.shape
    loss = torch.empty((b,), dtype=torch.float32, device=y_pred.device)
    _lib.check(_lib.load().tfrs_listwise_pairsum_fwd(kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l, temperature,
                                                      _lib.ptr(loss), _lib.current_stream()))
    ctx.save_for_backward(y_true, y_pred)
    ctx.args = (kind, temperature)
    return loss

  @staticmethod
  def backward(ctx, grad):
    from recommenders_amd import _lib
    y_true, y_pred = ctx.saved_tensors
    kind, temperature = ctx.args
    b, l = y_pred.shape
    scale = grad.to(torch.float32).contiguous()
    ds = torch.empty_like(y_pred)
    _lib.check(_lib.load().tfrs_listwise_pairsum_bwd(kind, _lib.ptr(y_true), _lib.ptr(y_pred), b, l, temperature,
                                                      _lib.ptr(scale), _lib.ptr(ds), _lib.current_stream()))
    return ds, None, None, None


class _PairSumLoss(_ListwiseLoss):
  """``temperature`` divides the scores (``alpha = float32(1 / temperature)``): it must be finite and positive and keep
  that reciprocal finite.  Pads are selected out (TF-Ranking pushes them to ``min - 1e3`` / ``log 1e-10``); there is no
  ``lambda_weight``, no per-item weight and no Gumbel variant."""

  def __init__(self, reduction, name, temperature):
    super().__init__(reduction, name)
    try:
      ok = not isinstance(temperature, bool) and 0.0 < float(temperature) < float("inf")      # (NaN fails both)
      if ok:      # as float32, as the C entry sees it
        t32 = torch.tensor(float(temperature), dtype=torch.float32)
        ok = bool(t32 > 0) and bool(torch.isfinite(t32)) and bool(torch.isfinite(1.0 / t32))
    except (TypeError, ValueError, OverflowError):
      ok = False
    if not ok:
      raise ValueError(f"{type(self).__name__}: temperature must be finite and positive, with a finite float32 "
                       f"reciprocal, got {temperature!r}")
    self.temperature = float(temperature)

  def _per_sample(self, y_true, y_pred):
    return _PairSumFn.apply(y_pred, y_true, self._KIND, self.temperature)


class ApproxNDCGLoss(_PairSumLoss):
  """``-(1 / IDCG) sum_i (2^{y_i} - 1) / log2(1 + r_i)`` over the valid items of a list: NDCG with every hard rank
  replaced by the soft rank ``r_i = 1 + sum_{j != i} sigmoid((s_j - s_i) / temperature)``.  ``IDCG`` is
  ``NDCGMetric``'s ideal DCG over all ranks; a list whose ``IDCG`` is not positive has loss and gradient 0 (TF-Ranking
  replaces such a list's labels by 1e-10)."""
  _KIND = _APPROX_NDCG

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "approx_ndcg_loss",
               temperature: float = 0.1):
    super().__init__(reduction, name, temperature)


class ApproxMRRLoss(_PairSumLoss):
  """``-(1 / sum y) sum_i y_i / r_i`` over the valid items of a list, ``r_i`` the soft rank of ``ApproxNDCGLoss``; a
  list whose labels sum to nothing positive has loss and gradient 0 (TF-Ranking gives it a non-zero value)."""
  _KIND = _APPROX_MRR

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "approx_mrr_loss",
               temperature: float = 0.1):
    super().__init__(reduction, name, temperature)


class UniqueSoftmaxLoss(_PairSumLoss):
  """``sum_i (2^{y_i} - 1) (lse_i - t_i)`` over the valid items of a list, ``t = s / temperature`` and
  ``lse_i = log(exp(t_i) + sum_{y_j < y_i} exp(t_j))``: every item competes only with the items labelled below it."""
  _KIND = _UNIQUE_SOFTMAX

  def __init__(self, reduction: str = "sum_over_batch_size", name: Optional[str] = "unique_softmax_loss",
               temperature: float = 1.0):
    super().__init__(reduction, name, temperature)
