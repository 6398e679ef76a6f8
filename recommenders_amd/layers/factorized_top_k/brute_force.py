"""``BruteForce``: exact top-K over a packed, layer-owned device index."""

import ctypes
from typing import Any, Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from recommenders_amd import _lib

from ._base import TopK
from ._common import (MAX_FUSED_DIM, MAX_FUSED_K, MAX_MERGE_HEADS, MAX_MERGE_PAIRS, NOT_INDEXED_MESSAGE, ArrayLike,
                      Tensor, _as_f32_matrix, _as_f32_queries, _check_candidates_with_identifiers,
                      _check_k_against_rows, _check_query_dim, _device, _host_identifiers, _Identifiers, _IndexHandle, _iter_blocks, _save_npz,
                      _validate_candidates, _wide_topk_update, _workspace)


_APPEND_CHUNK_ROWS = 1 << 20   # rows gathered before an index append (BruteForce.index_from_dataset)


class _Duplicates:
  """Bookkeeping of a de-duplicated index: ``start[u] .. start[u + 1]`` delimits, in ``rows``, the
  ascending original row numbers that distinct row ``u`` stands for; ``distinct_of_row[r]`` is the
  distinct row of original row ``r`` (to rebuild the corpus)."""

  def __init__(self, start: Tensor, rows: Tensor, distinct_of_row: Tensor, max_multiplicity: int):
    self.start, self.rows, self.distinct_of_row = start, rows, distinct_of_row
    self.count = int(start.numel() - 1)
    self.max_multiplicity = max_multiplicity


def _find_duplicates(cand: Tensor, min_multiplicity: int = 16, min_fraction: float = 0.1):
  """Groups bit-identical rows of ``cand`` (64-bit row hash from ``tfrs_row_hash64``, stable sort,
  exact comparison of hash neighbours -- a hash collision only costs a missed merge).  Returns
  ``(canonical_rows, _Duplicates)`` when de-duplication pays -- some row occurs at least
  ``min_multiplicity`` times or at least ``min_fraction`` of the rows are copies -- else ``None``.
  Index-time work: one pass over the rows, one sort of n 64-bit keys."""
  n, d = cand.shape
  if n < 2:
    return None
  lib = _lib.load()
  h = torch.empty((n,), dtype=torch.int64, device=cand.device)
  _lib.check(lib.tfrs_row_hash64(_lib.ptr(cand), n, d, _lib.ptr(h), _lib.current_stream()))
  hs, perm = torch.sort(h, stable=True)            # equal hashes: ascending original row
  same_hash = hs[1:] == hs[:-1]
  if not bool(same_hash.any()):
    return None
  # exact comparison, only where neighbouring hashes agree
  pos = torch.nonzero(same_hash).reshape(-1) + 1
  eq = torch.zeros((n,), dtype=torch.bool, device=cand.device)
  for lo in range(0, pos.numel(), 1 << 20):        # bounded temporaries
    p = pos[lo:lo + (1 << 20)]
    a, b = cand.index_select(0, perm[p]), cand.index_select(0, perm[p - 1])
    eq[p] = (a.view(torch.int32) == b.view(torch.int32)).all(dim=1)
  new_group = ~eq                                   # position 0 starts a group
  group = torch.cumsum(new_group.to(torch.int64), 0) - 1          # group of every sorted position
  n_groups = int(group[-1].item()) + 1
  sizes = torch.bincount(group, minlength=n_groups)
  max_mult = int(sizes.max().item())
  if n_groups == n or (max_mult < min_multiplicity and n - n_groups < min_fraction * n):
    return None
  # canonical (lowest) original row of every group; distinct rows are numbered by ascending
  # canonical row so that the distinct index keeps the corpus order
  first_pos = torch.nonzero(new_group).reshape(-1)
  canon = perm[first_pos]
  canon_sorted, by_canon = torch.sort(canon)
  rank_of_group = torch.empty_like(by_canon)
  rank_of_group[by_canon] = torch.arange(n_groups, device=cand.device)
  distinct_of_sorted = rank_of_group[group]
  distinct_of_row = torch.empty((n,), dtype=torch.int64, device=cand.device)
  distinct_of_row[perm] = distinct_of_sorted
  # rows grouped by distinct row, ascending within a group (stable sort of 0..n-1 by distinct row)
  _, rows = torch.sort(distinct_of_row, stable=True)
  counts = torch.bincount(distinct_of_row, minlength=n_groups)
  start = torch.zeros((n_groups + 1,), dtype=torch.int64, device=cand.device)
  start[1:] = torch.cumsum(counts, 0)
  return canon_sorted, _Duplicates(start.contiguous(), rows.to(torch.int32).contiguous(),
                                   distinct_of_row.to(torch.int32).contiguous(), max_mult)


def _raise_if_nonfinite_candidates(handle: _IndexHandle) -> None:
  """After the packer has run and the stream was synchronised: bit 0 of the handle's flag word."""
  if handle.flags() & 1:
    raise ValueError("The candidates contain NaN or Inf: the fp16-prefiltered search needs finite candidate rows "
                     "(its error bound is built from row norms; include/tfrs_hip.h).  Clean the embeddings -- a "
                     "diverged training run is the usual source -- before indexing them.")


class _IndexState:
  """Everything an ``index`` / ``index_from_dataset`` builds.  A layer holds ONE of these and replaces it as a
  whole, so nothing of a previous corpus survives a re-index: ``handle`` (the packed device index) or ``wide`` (the
  row-major copy of a corpus with d > 128), never both; ``dup`` for a de-duplicated index; ``plain`` and
  ``last_call`` are filled in by calls."""

  def __init__(self, handle: Optional[_IndexHandle] = None, wide: Optional[Tensor] = None, n: int = 0, d: int = 0,
               ids: Optional[_Identifiers] = None, dup: Optional[_Duplicates] = None):
    self.handle, self.wide, self.n, self.d, self.ids, self.dup = handle, wide, int(n), int(d), ids, dup
    self.plain: Optional["BruteForce"] = None     # un-de-duplicated copy for k > MAX_FUSED_K, built on demand
    self.last_call = None                         # (workspace, nq, k) of the last fused search, for the redo counts
    # rows held by the device index: the distinct rows of a de-duplicated corpus, else all
    self.index_rows = dup.count if dup is not None else self.n


class BruteForce(TopK):
  """Brute force retrieval (reference :515-610): exact top-K of ``q @ candidates^T``.

  ``index`` copies the candidates into a layer-owned, MFMA-friendly packed corpus in
  HBM (:559-584); ``call`` is one fused scan, the ``[B, N]`` score matrix is never
  materialised.

  Multi-head queries ``[B, H, D]`` (the max-sim queries of ``tasks.Retrieval``, tasks/retrieval.py:172-176; not in
  the reference's layer, which scores 2-D queries only): the score of a candidate is the max over the query's heads
  and the result is the exact top-k of that score under (score descending, row ascending).  The ``B * H`` flat rows
  are searched with the same ``k`` and ``tfrs_topk_merge_heads`` merges each query's ``H`` lists (the union of the
  per-head top-k lists contains the top-k of the max; csrc/topk_merge_heads.hip).  Envelope: ``H <= 32``,
  ``k <= 1024``, ``H * k <= 8192``, ``D <= 128``.  Rank-2 input keeps meaning a batch of single-head queries.

  ``dedup`` (default ``"auto"``; not in the reference): ``tf.math.top_k`` breaks ties by the lower
  index (:605), so on a corpus with many EXACT copies of a row (default / cold-start embeddings,
  popularity-weighted duplicates) every copy of a top-K row is a candidate for the K-th place, no
  score threshold separates them and the filtered scans degrade to their exact-recompute path
  (68x slower at BASELINE configs[1] shapes on a Zipf-duplicated corpus).  ``index`` therefore
  looks for bit-identical rows and, when some row occurs >= 16 times or >= 10 % of the rows are
  copies, indexes the DISTINCT rows only; a call searches those and expands the best of them back
  into the exact top-K of the original corpus (``tfrs_topk_expand_duplicates``: same scores, same
  row order as the full search).  ``False`` switches the detection off, ``True`` forces it for any
  duplicate.
  """

  def __init__(self, query_model: Optional[Callable] = None, k: int = 10,
               name: Optional[str] = None, dedup="auto", check_finite: bool = False):
    """``check_finite`` (not in the reference's signature): candidates and queries must be finite -- the reference's
    ``tf.math.top_k`` (:605) tolerates NaN / Inf scores, the fp16-prefiltered search here does not (include/tfrs_hip.h,
    ``tfrs_index_nonfinite``).  Non-finite CANDIDATES always raise ``ValueError`` from ``index`` /
    ``index_from_dataset``.  Non-finite QUERIES are recorded by the search kernels without a host synchronisation:
    only their own result rows are affected, and the ``ValueError`` is raised by the NEXT call (deferred, like an
    asynchronous device error); ``check_finite=True`` synchronises after every call and raises at once."""
    super().__init__(k=k, name=name)
    self.query_model = query_model
    self._check_finite = bool(check_finite)
    self._dedup = dedup
    self._state = _IndexState()

  # (read-only views of the index state under the names other layers and the tests use)
  _index = property(lambda self: self._state.handle)
  _n = property(lambda self: self._state.n)
  _d = property(lambda self: self._state.d)
  _ids = property(lambda self: self._state.ids)
  _dup = property(lambda self: self._state.dup)

  def _indexed(self) -> _IndexState:
    st = self._state
    if st.handle is None and st.wide is None:                           # :594-598
      raise ValueError(NOT_INDEXED_MESSAGE)
    return st

  def index(self, candidates: ArrayLike, identifiers: Optional[ArrayLike] = None) -> "BruteForce":
    cand = _validate_candidates(candidates, identifiers)                # :547-557
    n, d = cand.shape
    if d > MAX_FUSED_DIM:
      # embedding dims above 128: layer-owned row-major copy (:571-580), scored block by block
      # through the GEMM kernels (scores are GEMM sums, f32 accuracy)
      self._state = _IndexState(wide=cand.clone(), n=n, d=d, ids=_Identifiers(identifiers, n))
      return self
    dup, packed_rows = None, cand
    if self._dedup is True or (self._dedup and n >= 4096):
      found = (_find_duplicates(cand, 2, 0.0) if self._dedup is True else _find_duplicates(cand))
      if found is not None:
        canonical, dup = found
        packed_rows = cand.index_select(0, canonical)      # the distinct rows, in corpus order
    handle = _IndexHandle()
    _lib.check(handle._lib.tfrs_index_set(handle.handle, _lib.ptr(packed_rows), packed_rows.shape[0],
                                          packed_rows.shape[1], _lib.current_stream()))
    torch.cuda.current_stream().synchronize()  # `cand` may be a temporary upload
    _raise_if_nonfinite_candidates(handle)
    # the previous index (if any) is dropped
    self._state = _IndexState(handle=handle, n=n, d=d, ids=_Identifiers(identifiers, n), dup=dup)
    return self

  def index_from_dataset(self, candidates: Iterable, total_rows: Optional[int] = None) -> "BruteForce":
    """``TopK.index_from_dataset`` (:179-215).  With ``total_rows`` (the dataset's cardinality)
    the blocks are packed straight into a device index reserved once
    (``tfrs_index_reserve`` / ``tfrs_index_append``): peak memory is the packed index plus ONE
    block instead of the reference's ``tf.concat`` of every block (:196-215), which is what a
    corpus of 100 M rows needs.  Without it the blocks are concatenated like the reference."""
    if total_rows is None:
      return super().index_from_dataset(candidates)
    _check_candidates_with_identifiers(candidates)
    for _, first_block in _iter_blocks(candidates):
      if first_block.shape[1] > MAX_FUSED_DIM:
        return super().index_from_dataset(candidates)     # wide dims: plain row-major copy
      break
    handle, ids, n, d = None, [], 0, 0
    # The index stores every appended block in a pseudo-random row order (the filter bound is
    # taken from a sample of the stored stages, csrc/topk_api.hip), which only mixes rows WITHIN
    # a block: small dataset batches (`movies.batch(128)`) are therefore gathered into chunks of
    # >= _APPEND_CHUNK_ROWS rows before they are appended.  Row order, and with it the returned
    # identifiers, is unchanged.
    pending, pending_rows = [], 0

    def flush():
      nonlocal pending, pending_rows
      if not pending:
        return
      chunk = pending[0] if len(pending) == 1 else torch.cat(pending, dim=0)
      _lib.check(handle._lib.tfrs_index_append(handle.handle, _lib.ptr(chunk), chunk.shape[0],
                                               _lib.current_stream()))
      torch.cuda.current_stream().synchronize()   # the blocks may be temporary uploads
      pending, pending_rows = [], 0

    for block_ids, block in _iter_blocks(candidates):
      if block_ids is not None:
        ids.append(_host_identifiers(block_ids))
      block = _as_f32_matrix(block, "candidates")
      if handle is None:
        d = block.shape[1]
        handle = _IndexHandle()
        _lib.check(handle._lib.tfrs_index_reserve(handle.handle, int(total_rows), d,
                                                  _lib.current_stream()))
      elif block.shape[1] != d:
        raise ValueError(f"Candidate blocks disagree on the embedding dimension ({block.shape[1]} vs {d}).")
      if n + block.shape[0] > total_rows:
        raise ValueError(f"The dataset holds more than total_rows={total_rows} candidates.")
      pending.append(block)
      pending_rows += block.shape[0]
      n += block.shape[0]
      if pending_rows >= _APPEND_CHUNK_ROWS:
        flush()
    if handle is None:
      raise ValueError("The candidate dataset is empty.")
    flush()
    _raise_if_nonfinite_candidates(handle)
    # (streamed ingest: blocks are indexed as they come, so no de-duplication)
    self._state = _IndexState(handle=handle, n=n, d=d,
                              ids=_Identifiers(np.concatenate(ids, axis=0) if ids else None, n))
    return self

  def _embed(self, queries) -> Tensor:
    if self.query_model is not None:
      queries = self.query_model(queries)
    return _as_f32_queries(queries)

  def _query_rows_heads(self, q: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """Multi-head queries ``[B, H, D]``: top-k of ``max_h q_bh . c`` -- the flat rows' top-k lists, merged per query."""
    st = self._state
    nq, heads, d = q.shape
    if d != st.d:
      raise ValueError(f"Query dimension {d} does not match the index ({st.d}).")
    _check_k_against_rows(k, st.n)
    if not 1 <= heads <= MAX_MERGE_HEADS:
      raise ValueError(f"BruteForce: multi-head queries take 1 to {MAX_MERGE_HEADS} heads (got {heads}).")
    if st.wide is not None:
      raise ValueError(f"BruteForce: multi-head queries need an embedding dim of at most {MAX_FUSED_DIM} (index: {d}).")
    if k > MAX_FUSED_K:
      raise ValueError(f"BruteForce: multi-head queries take k <= {MAX_FUSED_K} (got k={k}).")
    if heads * k > MAX_MERGE_PAIRS:
      raise ValueError(f"BruteForce: heads * k = {heads * k} is above the {MAX_MERGE_PAIRS} (score, row) pairs the "
                       f"multi-head merge holds per query.")
    scores, rows = self._query_rows(q.reshape(nq * heads, d), k, embedded=True)
    if heads == 1:
      return scores, rows
    out_s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    out_r = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    _lib.check(_lib.load().tfrs_topk_merge_heads(_lib.ptr(scores), _lib.ptr(rows), nq, heads, k, k,
                                                 _lib.ptr(out_s), _lib.ptr(out_r), _lib.current_stream()))
    return out_s, out_r

  def _query_rows(self, queries, k: int, embedded: bool = False) -> Tuple[Tensor, Tensor]:
    st = self._indexed()
    q = queries if embedded else self._embed(queries)                   # :600-601
    if q.dim() == 3:
      return self._query_rows_heads(q, k)
    _check_query_dim(q, st.d)
    _check_k_against_rows(k, st.n)
    lib = _lib.load()
    nq = q.shape[0]
    if st.wide is not None:
      scores = torch.zeros((nq, k), dtype=torch.float32, device=q.device)
      rows = torch.zeros((nq, k), dtype=torch.int32, device=q.device)
      _wide_topk_update(q, st.wide, 0, k, scores, rows, 0)
      st.last_call = None
      return scores, rows
    if k > MAX_FUSED_K:
      if st.dup is not None:     # pages + expansion: (rare) search a plain copy of the corpus
        if st.plain is None:
          st.plain = BruteForce(k=self._k, dedup=False).index(self.candidates())
        return st.plain._query_rows_paged(q, k)
      return self._query_rows_paged(q, k)
    self._raise_if_nonfinite_queries()             # (deferred: recorded by an EARLIER call's kernels)
    kk = min(k, st.index_rows)                      # (de-duplicated: the best kk DISTINCT rows)
    scores = torch.empty((nq, kk), dtype=torch.float32, device=q.device)
    rows = torch.empty((nq, kk), dtype=torch.int32, device=q.device)
    ws = _workspace(lib.tfrs_bruteforce_topk_workspace_bytes(nq, st.index_rows, st.d, kk))
    _lib.check(lib.tfrs_bruteforce_topk(
        st.handle.handle, _lib.ptr(q), nq, kk, _lib.ptr(scores), _lib.ptr(rows),
        _lib.ptr(ws), ws.numel(), _lib.current_stream()))               # :603-605
    st.last_call = (ws, nq, kk)
    if self._check_finite:
      torch.cuda.current_stream().synchronize()
      self._raise_if_nonfinite_queries()
    if st.dup is None:
      return scores, rows
    # every original row is a candidate with its distinct row's score: exact top-k of the corpus
    out_s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    out_r = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    _lib.check(lib.tfrs_topk_expand_duplicates(
        _lib.ptr(scores), _lib.ptr(rows), nq, kk, _lib.ptr(st.dup.start), _lib.ptr(st.dup.rows), k,
        _lib.ptr(out_s), _lib.ptr(out_r), _lib.current_stream()))
    return out_s, out_r

  def _query_rows_paged(self, q: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """``k`` beyond the selection kernels' 1024 slots (``tf.math.top_k`` has no limit, :605): pages
    of up to 1024 results, each the best rows strictly after the previous page's last (score, row)
    in the result order (``tfrs_bruteforce_topk_below``); the pages are written side by side into
    the ``[B, k]`` outputs, which are therefore exactly the sorted top-k.  One all-f32 scan of the
    corpus per page.  (``_query_rows`` has checked ``k`` against the corpus.)"""
    st = self._state
    lib = _lib.load()
    nq = q.shape[0]
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    rows = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    ws = _workspace(lib.tfrs_bruteforce_topk_below_workspace_bytes(nq, st.n, st.d, MAX_FUSED_K))
    page_s = torch.empty((nq, MAX_FUSED_K), dtype=torch.float32, device=q.device)
    page_r = torch.empty((nq, MAX_FUSED_K), dtype=torch.int32, device=q.device)
    done = 0
    while done < k:
      kk = min(MAX_FUSED_K, k - done)
      ps, pr = (page_s, page_r) if kk == MAX_FUSED_K else (page_s[:, :kk].contiguous(), page_r[:, :kk].contiguous())
      last_s = None if done == 0 else scores[:, done - 1:]        # row stride k: element [q, done - 1]
      last_r = None if done == 0 else rows[:, done - 1:]
      _lib.check(lib.tfrs_bruteforce_topk_below(
          st.handle.handle, _lib.ptr(q), nq, kk,
          None if last_s is None else ctypes.c_void_p(last_s.data_ptr()),
          None if last_r is None else ctypes.c_void_p(last_r.data_ptr()), k,
          _lib.ptr(ps), _lib.ptr(pr), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
      scores[:, done:done + kk] = ps
      rows[:, done:done + kk] = pr
      done += kk
    st.last_call = None
    return scores, rows

  def nonfinite_flags(self, reset: int = 0) -> int:
    """The index handle's flag word (``tfrs_index_nonfinite``): bit 0 non-finite candidates, bit 1 non-finite
    queries in a call whose kernels have completed.  Reading it does not synchronise."""
    handle = self._state.handle
    return 0 if handle is None else handle.flags(reset)

  def _raise_if_nonfinite_queries(self) -> None:
    if self.nonfinite_flags() & 2:
      self.nonfinite_flags(reset=2)
      raise ValueError("BruteForce: the queries of this or an earlier call contained NaN or Inf (or a row norm beyond "
                       "the float32 range): the result rows of those queries hold non-finite scores and unspecified "
                       "indices; every other row is exact.  Queries must be finite (include/tfrs_hip.h).")

  def last_redo_count(self) -> int:
    """Queries of the most recent ``call`` that were answered by the exact-recompute path of
    the fp16-prefiltered search (0 on well-behaved data).  Synchronises the stream."""
    st = self._state
    if st.last_call is None:
      return 0
    ws, nq, k = st.last_call
    out = ctypes.c_int32(0)
    _lib.check(_lib.load().tfrs_bruteforce_topk_redo_count(
        _lib.ptr(ws), nq, st.index_rows, k, ctypes.byref(out), _lib.current_stream()))
    return int(out.value)

  def last_redo_reasons(self) -> dict:
    """``last_redo_count`` split by cause (include/tfrs_hip.h).  Synchronises the stream."""
    names = ("list_overflow", "statistical_bound", "retained_set", "longest_list")
    st = self._state
    if st.last_call is None:
      return dict.fromkeys(names, 0)
    ws, nq, k = st.last_call
    out = (ctypes.c_int32 * 4)()
    _lib.check(_lib.load().tfrs_bruteforce_topk_redo_reasons(
        _lib.ptr(ws), nq, st.index_rows, k, out, _lib.current_stream()))
    return {name: int(out[i]) for i, name in enumerate(names)}

  def call(self, queries, k: Optional[int] = None):
    scores, rows = self._query_rows(queries, self._k_or_default(k))
    return scores, self._state.ids.gather(rows)                         # :607

  def make_graphed_call(self, example_queries, k: Optional[int] = None):
    """``call`` for a fixed batch shape, captured once in a HIP graph and replayed (``TopK._graphed_call``).

    A small-batch query is a chain of ~8 short kernels (query norms, threshold pass, filter
    pass, exact re-scoring); replaying them from a graph removes the per-launch host cost that
    dominates the latency of single queries.  The index must not be re-indexed afterwards."""
    if self._indexed().wide is not None:
      raise NotImplementedError("make_graphed_call: embedding dims above 128 use per-block launches")
    return self._graphed_call(example_queries, self._k_or_default(k))

  def candidates(self) -> Tensor:
    """The indexed candidate matrix (unpacked copy), for checkpointing."""
    st = self._indexed()
    if st.wide is not None:
      return st.wide.clone()
    out = torch.empty((st.index_rows, st.d), dtype=torch.float32, device=_device())
    _lib.check(_lib.load().tfrs_index_unpack(st.handle.handle, _lib.ptr(out), _lib.current_stream()))
    if st.dup is not None:       # every original row from its distinct row
      out = out.index_select(0, st.dup.distinct_of_row.long())
    return out

  def is_exact(self) -> bool:
    return True

  # -- persistence (the role of SavedModel export in the reference, --------------------------
  #    factorized_top_k_test.py:152-165, basic_retrieval.ipynb "serving") ---------------------
  def state_dict(self) -> Dict[str, Any]:   # type: ignore[override]
    """Everything needed to rebuild the index: the row-major float32 candidates (unpacked from
    the device images), the identifiers (``None`` = row numbers) and ``k``."""
    return {"candidates": self.candidates().cpu().numpy(), "identifiers": self._indexed().ids.host_values(),
            "k": self._k}

  def load_state_dict(self, state: Dict[str, Any]) -> "BruteForce":   # type: ignore[override]
    self._k = int(state.get("k", self._k))
    return self.index(state["candidates"], state.get("identifiers"))

  def save(self, path: str) -> None:
    """Writes the index to one ``.npz`` file (string identifiers are stored as a unicode array)."""
    _save_npz(path, self.state_dict())

  @classmethod
  def load(cls, path: str, query_model: Optional[Callable] = None) -> "BruteForce":
    with np.load(path, allow_pickle=False) as f:
      layer = cls(query_model=query_model, k=int(f["k"]))
      return layer.index(f["candidates"], f["identifiers"] if "identifiers" in f.files else None)
