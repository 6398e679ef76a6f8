"""Listwise ranking metrics (state on the device, ``update_state`` / ``result`` / ``reset_states`` like the others)."""

from typing import Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.metrics.factorized_top_k import Mean


class NDCGMetric(Mean):
  """Normalised discounted cumulative gain of ``[batch, list]`` scores against graded labels (``-1`` pads), gain
  ``2^y - 1``, discount ``1 / log2(rank + 2)``, cut at ``topn``; the weighted mean over the lists whose ideal DCG is
  positive, 0 when there is none.  One fused kernel per update (``tfrs_listwise_ndcg``); the running
  sum and count are updated in place, so a captured step replays them."""

  def __init__(self, name: str = "ndcg_metric", topn: Optional[int] = None):
    super().__init__(name)
    if topn is not None and (int(topn) != topn or topn < 1):
      raise ValueError(f"NDCGMetric: topn must be a positive integer or None, got {topn!r}")
    self.topn = None if topn is None else int(topn)

  def update_state(self, y_true, y_pred, sample_weight=None):
    from recommenders_amd.losses import _listwise_inputs
    y_true, y_pred = _listwise_inputs(y_true, y_pred, "NDCGMetric", sample_weight)
    b, l = y_pred.shape
    if b == 0:
      return
    out = torch.zeros((2, b), dtype=torch.float32, device=y_pred.device)     # per-list NDCG, counted
    topn = 0 if self.topn is None else min(self.topn, 2 ** 31 - 1)
    _lib.check(_lib.load().tfrs_listwise_ndcg(_lib.ptr(y_true), _lib.ptr(y_pred), b, l, topn, _lib.ptr(out[0]),
                                              _lib.ptr(out[1]), _lib.current_stream()))
    counted = out[1]
    if sample_weight is not None:
      counted = counted * torch.as_tensor(sample_weight).reshape(-1).to(counted.device, torch.float32)
    super().update_state(out[0], counted)
