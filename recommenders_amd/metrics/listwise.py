"""Listwise ranking metrics (state on the device, ``update_state`` / ``result`` / ``reset_states`` like the others).

Every class here is one ``(kind, topn)`` of ``tfrs_listwise_metrics`` (csrc/listwise.hip; formulas: DESIGN 4.24 for NDCG,
4.26 for the rest): ``y_true`` / ``y_pred`` are ``[batch, list]``, a position is valid iff its label is ``>= 0`` (``-1``
pads), an item is *relevant* iff its label is ``>= 1``, ranks follow the scores descending with ties by position
ascending, and ``topn`` cuts the ranking (``None``: no cut).  The kernel gives a value and a non-negative weight per list;
a metric's result is the ``Mean`` of the values under weight x ``sample_weight`` (per list, ``[B]`` or ``[B, 1]``), 0 when
nothing counts.  ``update_listwise_metrics`` updates several metrics from one launch."""

import ctypes
from typing import List, Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.metrics.factorized_top_k import Mean

MAX_METRICS_PER_CALL = 16         # TFRS_LISTWISE_METRIC_MAX
_NDCG, _DCG, _MRR, _HITS, _PRECISION, _RECALL, _MAP, _ARP, _OPA = range(9)


def _launch(descriptors, y_true, y_pred, values, weights):
  """One ``tfrs_listwise_metrics`` call: ``descriptors`` = up to 16 ``(kind, topn or None)``; ``values`` / ``weights``
  are contiguous ``[len(descriptors), B]`` float32."""
  n = len(descriptors)
  kinds = (ctypes.c_int * n)(*[k for k, _ in descriptors])
  topns = (ctypes.c_int * n)(*[0 if t is None else min(t, 2 ** 31 - 1) for _, t in descriptors])
  b, l = y_pred.shape
  _lib.check(_lib.load().tfrs_listwise_metrics(_lib.ptr(y_true), _lib.ptr(y_pred), b, l, n, kinds, topns,
                                               _lib.ptr(values), _lib.ptr(weights), _lib.current_stream()))


def _per_list(descriptors, y_true, y_pred):
  """``[2, M, B]``: per descriptor and list the value and the weight; one launch per 16 descriptors."""
  m = len(descriptors)
  out = torch.zeros((2, m, y_pred.shape[0]), dtype=torch.float32, device=y_pred.device)
  for lo in range(0, m, MAX_METRICS_PER_CALL):
    hi = min(lo + MAX_METRICS_PER_CALL, m)
    _launch(descriptors[lo:hi], y_true, y_pred, out[0, lo:hi], out[1, lo:hi])
  return out


class _ListMetric(Mean):
  """A ``Mean`` over the lists of one ``(kind, topn)``: input checks, the one-metric call, the in-place state."""

  _KIND = None

  def __init__(self, name: str, topn: Optional[int] = None):
    super().__init__(name)
    if topn is not None and (int(topn) != topn or topn < 1):
      raise ValueError(f"{type(self).__name__}: topn must be a positive integer or None, got {topn!r}")
    self.topn = None if topn is None else int(topn)
    self._group = None              # the state buffer shared with the other metrics of update_listwise_metrics

  def update_state(self, y_true, y_pred, sample_weight=None):
    from recommenders_amd.losses import _listwise_inputs
    y_true, y_pred = _listwise_inputs(y_true, y_pred, type(self).__name__, sample_weight)
    b = y_pred.shape[0]
    if b == 0:
      return
    out = torch.zeros((2, b), dtype=torch.float32, device=y_pred.device)     # per-list value, weight
    _launch([(self._KIND, self.topn)], y_true, y_pred, out[0], out[1])
    weight = out[1]
    if sample_weight is not None:
      weight = weight * torch.as_tensor(sample_weight).reshape(-1).to(weight.device, torch.float32)
    super().update_state(out[0], weight)


class NDCGMetric(_ListMetric):
  """Normalised discounted cumulative gain of ``[batch, list]`` scores against graded labels (``-1`` pads), gain
  ``2^y - 1``, discount ``1 / log2(rank + 2)``, cut at ``topn``; the weighted mean over the lists whose ideal DCG is
  positive, 0 when there is none.  One fused kernel per update (``tfrs_listwise_metrics``); the running
  sum and count are updated in place, so a captured step replays them."""

  _KIND = _NDCG

  def __init__(self, name: str = "ndcg_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class DCGMetric(_ListMetric):
  """Discounted cumulative gain, ``sum_{r < min(n, topn)} (2^y - 1) / log2(r + 2)`` in score order: NDCG's numerator,
  term for term.  The mean over the lists with some label ``> 0``."""

  _KIND = _DCG

  def __init__(self, name: str = "dcg_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class MRRMetric(_ListMetric):
  """Mean reciprocal rank: ``1 / (rank of the first relevant item)`` (1-based) if it lies within ``topn``, else 0.  The
  mean over the lists that hold a relevant item."""

  _KIND = _MRR

  def __init__(self, name: str = "mrr_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class HitsMetric(_ListMetric):
  """Hit rate: 1 if a relevant item ranks within ``topn``, else 0.  The mean over the lists that hold a relevant item."""

  _KIND = _HITS

  def __init__(self, name: str = "hits_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class PrecisionMetric(_ListMetric):
  """Precision: the relevant items within ``topn`` over ``min(topn, L)``.  As in TF-Ranking the denominator is the cut or
  the PADDED list width ``L`` (``topn=None``: ``L``), not the number of valid items, so padding a batch wider lowers it.
  The mean over the lists that hold a relevant item."""

  _KIND = _PRECISION

  def __init__(self, name: str = "precision_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class RecallMetric(_ListMetric):
  """Recall: the relevant items within ``topn`` over the relevant items of the list.  The mean over the lists that hold
  a relevant item."""

  _KIND = _RECALL

  def __init__(self, name: str = "recall_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class MeanAveragePrecisionMetric(_ListMetric):
  """Mean average precision: ``sum over the relevant ranks r < min(n, topn) of c_r / (r + 1)``, ``c_r`` the relevant
  items at ranks ``<= r``, over the relevant items of the list.  The mean over the lists that hold a relevant item."""

  _KIND = _MAP

  def __init__(self, name: str = "map_metric", topn: Optional[int] = None):
    super().__init__(name, topn)


class ARPMetric(_ListMetric):
  """Average relevance position: ``sum y (rank + 1) / sum y`` pooled over all lists (a list's weight is its ``sum y``),
  ranks 1-based; lower is better."""

  _KIND = _ARP

  def __init__(self, name: str = "arp_metric"):
    super().__init__(name, None)


class OPAMetric(_ListMetric):
  """Ordered pair accuracy: of the pairs with ``y_i > y_j``, the share with ``s_i > s_j`` (tied scores count as wrong),
  pooled over all lists (a list's weight is its number of such pairs)."""

  _KIND = _OPA

  def __init__(self, name: str = "opa_metric"):
    super().__init__(name, None)


class _Group:
  """``[3, M]`` on the device -- totals, counts, and the result row that ``Mean._bind`` asks for (unused here: the result
  is formed from total and count) -- whose columns the ``Mean``s of one metric list are bound to, so that one in-place
  add updates them all."""

  def __init__(self, members: List[_ListMetric], device):
    self.members = list(members)
    self.state = torch.zeros((3, len(members)), dtype=torch.float32, device=device)
    for i, metric in enumerate(self.members):
      metric._bind(self.state[0, i], self.state[1, i], self.state[2, i])      # (carries an existing state over)
      metric._group = self

  def holds(self, members, device) -> bool:
    return (self.state.device == device and len(members) == len(self.members) and
            all(a is b and a._group is self for a, b in zip(members, self.members)))


def update_listwise_metrics(metric_list, y_true, y_pred, sample_weight=None) -> None:
  """``update_state(y_true, y_pred, sample_weight)`` of every list metric in ``metric_list`` from ONE kernel launch
  (one per 16 metrics): the lists are loaded and sorted by score once for all of them.  The per-list values are then
  weighted and reduced for all metrics together and added to their states with one in-place add -- a fixed number of
  torch operations, whatever the number of metrics -- so a captured step replays.  Each metric ends in exactly the
  state its own ``update_state`` would have given it up to float32 rounding of the sums.

  The metrics of a list share one state buffer, made at the first call with that list (an existing state is carried
  over).  Calling with the same metrics in another list or order moves them to a new buffer: keep the list as it is once
  a step that contains this call has been captured, or the captured graph goes on adding to the old one."""
  members = list(metric_list)
  for metric in members:
    if not isinstance(metric, _ListMetric):
      raise TypeError(f"update_listwise_metrics: {metric!r} is not a listwise metric of recommenders_amd.metrics")
  if len(set(map(id, members))) != len(members):
    raise ValueError("update_listwise_metrics: a metric is listed twice")
  if not members:
    return
  from recommenders_amd.losses import _listwise_inputs
  y_true, y_pred = _listwise_inputs(y_true, y_pred, "update_listwise_metrics", sample_weight)
  b = y_pred.shape[0]
  if b == 0:
    return
  out = _per_list([(metric._KIND, metric.topn) for metric in members], y_true, y_pred)
  group = members[0]._group
  if group is None or not group.holds(members, y_pred.device):
    group = _Group(members, y_pred.device)
  if sample_weight is not None:
    out[1].mul_(torch.as_tensor(sample_weight).reshape(1, -1).to(out.device, torch.float32))
  out[0].mul_(out[1])
  # in place, like Mean.update_state: a captured step accumulates into this very storage
  group.state[:2].add_(out.sum(dim=2))
  for metric in members:
    metric._result_fresh = False
