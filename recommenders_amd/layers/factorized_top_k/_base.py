"""``TopK``: the interface of the top-K layers and the host code they share."""

import abc
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from ._common import (ArrayLike, Tensor, _Identifiers, _as_f32_matrix, _check_candidates_with_identifiers, _exclude,
                      _host_identifiers, _iter_blocks)


class TopK(torch.nn.Module, abc.ABC):
  """Interface for top K layers (reference :140-333).

  Implementers provide ``index`` (build the retrieval index from a candidate
  matrix) and ``call`` (top K candidates for a batch of queries).
  """

  def __init__(self, k: int, **kwargs) -> None:
    name = kwargs.pop("name", None)
    super().__init__()
    self.name = name if name is not None else type(self).__name__.lower()
    self._k = k
    self.query_model = None      # (the layers that take one set it)

  def _k_or_default(self, k: Optional[int]) -> int:
    return k if k is not None else self._k

  @abc.abstractmethod
  def index(self, candidates: ArrayLike, identifiers: Optional[ArrayLike] = None) -> "TopK":
    """Builds the retrieval index; an existing index is dropped (:158-177)."""
    raise NotImplementedError()

  def index_from_dataset(self, candidates: Iterable) -> "TopK":
    """Builds the index from an iterable of candidate blocks or (identifier block,
    candidate block) pairs (:179-215)."""
    _check_candidates_with_identifiers(candidates)
    blocks, ids = [], []
    for block_ids, block in _iter_blocks(candidates):
      if block_ids is not None:
        ids.append(_host_identifiers(block_ids))
      blocks.append(_as_f32_matrix(block, "candidates"))
    if not blocks:
      raise ValueError("The candidate dataset is empty.")
    return self.index(torch.cat(blocks, dim=0), np.concatenate(ids, axis=0) if ids else None)

  @abc.abstractmethod
  def call(self, queries, k: Optional[int] = None):
    """Returns (top scores [B, k], top identifiers [B, k]) (:217-240)."""
    raise NotImplementedError()

  def forward(self, queries, k: Optional[int] = None):
    return self.call(queries, k=k)

  def query_with_exclusions(self, queries, exclusions: ArrayLike, k: Optional[int] = None):
    """Top-k with per-query excluded identifiers (:242-288): query ``k + E``, then
    ``_exclude``."""
    k = self._k_or_default(k)
    num_excl = (exclusions.shape[1] if hasattr(exclusions, "shape")
                else np.asarray(exclusions).shape[1])
    adjusted_k = k + num_excl                                         # :286
    scores, rows = self._query_rows(queries, adjusted_k)               # :287
    return _exclude(scores, rows, self._identifier_table(), exclusions, k)   # :288

  @abc.abstractmethod
  def is_exact(self) -> bool:
    raise NotImplementedError()

  # -- implementation hooks -------------------------------------------------------------
  @abc.abstractmethod
  def _query_rows(self, queries, k: int) -> Tuple[Tensor, Tensor]:
    """(scores, int32 row numbers) before the identifier gather."""

  def _identifier_table(self) -> _Identifiers:
    """The table that turns the rows of the last ``_query_rows`` into identifiers."""
    return self._ids

  def _embed(self, queries) -> Tensor:
    if self.query_model is not None:
      queries = self.query_model(queries)
    return _as_f32_matrix(queries, "queries")

  def _graphed_call(self, example_queries, k: int):
    """``call`` for a fixed batch shape, captured once in a HIP graph and replayed: ``query_model`` (if any) and the
    identifier lookup stay outside the graph; the search itself -- same kernels, same results -- is inside.  Returns
    ``f(queries) -> (scores, identifiers)``; the returned score tensor is overwritten by the next call.  For layers
    whose ``_query_rows`` takes ``embedded=True`` and does not synchronise."""
    static_q = self._embed(example_queries).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for _ in range(2):
        self._query_rows(static_q, k, embedded=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      scores, rows = self._query_rows(static_q, k, embedded=True)

    def graphed(queries):
      q = self._embed(queries)
      if q.shape != static_q.shape:
        raise ValueError(f"graphed call was captured for queries of shape {tuple(static_q.shape)}; "
                         f"got {tuple(q.shape)}")
      static_q.copy_(q, non_blocking=True)
      graph.replay()
      return scores, self._identifier_table().gather(rows)

    graphed.graph = graph
    return graphed
