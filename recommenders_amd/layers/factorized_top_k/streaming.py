"""``Streaming``: exact top-K over a candidate stream that is re-read on every call."""

import ctypes
from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch

from recommenders_amd import _lib

from ._base import TopK
from ._common import (_INT32_MAX, _RAW_DIMS, _RAW_MAX_BLOCKS, BATCH_TOO_SMALL_MESSAGE, MAX_FUSED_DIM, MAX_FUSED_K,
                      NOT_INDEXED_MESSAGE, Tensor, _as_f32_matrix, _check_candidates_with_identifiers, _Identifiers,
                      _IndexHandle, _iter_blocks, _wide_topk_update, _workspace)
from .brute_force import BruteForce


class Streaming(TopK):
  """Retrieves the K highest scoring items from a large candidate stream
  (reference :336-512).  Keeps only a reference to the candidate iterable and
  re-reads it on every call; the running state is ``[B, <=K]`` in HBM.

  ``cache_packed_blocks`` (default on; not in the reference): when the candidates are a
  **list / tuple of GPU-resident tensors** (the serving case: device blocks held by the caller),
  the packed f32 + fp16 images built from them are kept between calls in ONE device index --
  rows in stream order, so global row numbers are the reference's counter (:477-488) -- and a
  call is then exactly ``BruteForce.call`` on it: no re-upload, no re-pack, no per-block
  threshold pass.  The cache keeps the tensor objects it packed alive and compares object
  identity, storage pointer and version counter on every call, so an address recycled by the
  allocator for a *new* tensor can never match.  Never cached (block-by-block path, device
  footprint of one block, exactly the reference's behaviour): lazily mapped / generated
  datasets (e.g. ``candidates.map(item_model)``: re-embedded on every pass), host arrays,
  tensors that take part in autograd (parameters, outputs with a ``grad_fn``), and corpora
  whose packed images would exceed ``cache_max_bytes`` (default 64 GiB).  Detached views of a
  trained table are safe: this package's fused optimizer kernels bump the table's version
  counter after writing through raw pointers.  A block written in place by a foreign raw
  kernel or through ``.data`` after the first call must be re-announced with
  ``index_from_dataset``.
  The cache holds 2.1x the candidate bytes (1.6x at dim 128).
  """

  def __init__(self, query_model: Optional[Callable] = None, k: int = 10,
               handle_incomplete_batches: bool = True,
               num_parallel_calls: Optional[int] = None, sorted_order: bool = True,
               cache_packed_blocks: bool = True, cache_max_bytes: int = 64 << 30,
               group_max_bytes: Optional[int] = None) -> None:
    super().__init__(k=k)
    self.query_model = query_model
    self._candidates = None
    self._handle_incomplete_batches = handle_incomplete_batches
    # `num_parallel_calls` / `sorted_order` (reference :343-350, :503: tf.data's parallel map and the
    # `sorted=` flag of tf.math.top_k) are accepted for API parity and have no effect here: the
    # blocks of a group are scored by one launch, and results always come back sorted
    self._num_parallel_calls = num_parallel_calls
    self._sorted = sorted_order
    # candidate bytes (float32 rows) searched per library call on the block-by-block path: the
    # blocks of a group are read IN PLACE (tfrs_streaming_topk_update_blocks), so this bounds how
    # many lazily produced blocks are alive at once plus the fp16 image of the group
    # rows kept alive per group of lazily produced blocks (+ their fp16 image for large batches): by default an
    # eighth of the device memory that is free at the first call, at most 8 GiB (a fixed 8 GiB
    # ran a `.map(model)` dataset out of memory on a busy GPU where the one-block-at-a-time path had fitted)
    self._group_max_bytes = None if group_max_bytes is None else max(int(group_max_bytes), 1)
    self._last_ids: Optional[_Identifiers] = None
    self._cache_blocks = cache_packed_blocks
    self._cache_max_bytes = int(cache_max_bytes)
    self._cache_key = None
    self._cache: Optional[BruteForce] = None
    self._cache_alive = None
    self._probe_fast = None
    self._base_row = 0
    self._finite: Optional[_IndexHandle] = None   # deferred finiteness record of the block-by-block path

  def index_from_dataset(self, candidates: Iterable) -> "Streaming":
    _check_candidates_with_identifiers(candidates)                     # :386
    self._candidates = candidates                                      # :388
    self._cache_key, self._cache, self._cache_alive, self._probe_fast = None, None, None, None
    return self

  def index(self, candidates, identifiers=None) -> "Streaming":
    """Not implemented. Please call `index_from_dataset` instead (:392-402)."""
    raise NotImplementedError(
        "The streaming top k class only accepts datasets. "
        "Please call `index_from_dataset` instead.")

  def _identifier_table(self) -> _Identifiers:
    return self._last_ids

  # -- cached path ---------------------------------------------------------------------------
  @staticmethod
  def _cacheable(t) -> bool:
    """A tensor whose content the cache may assume stable while (object, storage, version) are:
    resident f32/integer data that is not part of an autograd graph."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
            and not t.requires_grad and t.grad_fn is None)

  def _block_keys(self):
    """(key, blocks, ids) when the source is a list / tuple of cacheable GPU tensors, else None.
    Never iterates a lazy dataset (that would materialise it) and never touches the device.
    ``key`` holds the tensor OBJECTS (kept alive by the cache) next to their storage pointers
    and version counters: identity is part of the comparison, so a recycled address of a
    dead tensor cannot match."""
    src = self._candidates
    if not isinstance(src, (list, tuple)) or len(src) == 0:
      return None
    fast = self._probe_fast
    if fast is not None and fast[0] is src and len(src) == len(fast[1]):
      same = True
      for element, (ref, tensors) in zip(src, fast[1]):
        if element is not ref:
          same = False
          break
        for t, ptr, ver in tensors:
          if t._version != ver or t.data_ptr() != ptr:
            same = False
            break
        if not same:
          break
      if same:
        return fast[2]
    self._probe_fast = None
    if any(isinstance(element, (tuple, list)) and len(element) != 2 for element in src):
      return None
    keys, blocks, ids, seen = [], [], [], []
    for element, (block_ids, block) in zip(src, _iter_blocks(src)):
      if not (self._cacheable(block) and block.dim() == 2 and block.dtype == torch.float32):
        return None
      tensors = [(block, block.data_ptr(), block._version)]
      if block_ids is not None:
        if not self._cacheable(block_ids):
          return None     # host identifiers may change silently between calls
        tensors.append((block_ids, block_ids.data_ptr(), block_ids._version))
      keys.append(tuple((id(t), ptr, tuple(t.shape), ver) for t, ptr, ver in tensors))
      blocks.append(block)
      ids.append(block_ids)
      seen.append((element, tensors))
    d = blocks[0].shape[1]
    packed = sum(b.shape[0] for b in blocks) * (d * 6 + 32 + 4)    # f32 + fp16 images + row map
    if packed > self._cache_max_bytes:
      return None
    result = (tuple(keys), blocks, ids)
    self._probe_fast = (src, seen, result)
    return result

  def _cached_index(self, k: int) -> Optional["BruteForce"]:
    if not self._cache_blocks:
      return None
    if torch.cuda.is_current_stream_capturing():
      # a captured step (Model.fit / evaluate replay HIP graphs) runs no host code on replay, so the
      # (object, storage, version) comparison below could never notice that a block changed: under
      # capture the blocks are read in place, as the reference re-reads its dataset on every call
      return None
    probe = self._block_keys()
    if probe is None:
      self._cache_key, self._cache, self._cache_alive = None, None, None
      return None
    key, blocks, ids = probe
    if not self._handle_incomplete_batches and any(b.shape[0] < k for b in blocks):   # :431-436
      raise ValueError(BATCH_TOO_SMALL_MESSAGE.format(k=k))
    if key != self._cache_key:
      total = sum(b.shape[0] for b in blocks)
      if self._base_row + total > _INT32_MAX:
        raise ValueError("Streaming: global row numbers exceed int32 (base_row + rows = %d)"
                         % (self._base_row + total))
      bf = BruteForce(k=self._k)
      bf.index_from_dataset(list(zip(ids, blocks)) if ids[0] is not None else blocks, total_rows=total)
      # the packed tensors stay referenced for as long as their images are served: id() in the
      # key is only meaningful while the object lives
      self._cache_key, self._cache, self._cache_alive = key, bf, (blocks, ids)
    return self._cache

  def _query_rows(self, queries, k: int) -> Tuple[Tensor, Tensor]:
    if self._candidates is None:                                        # :412-416
      raise ValueError(NOT_INDEXED_MESSAGE)
    q = self._embed(queries)                                            # :418-419
    cached = self._cached_index(k)
    if cached is None and k > MAX_FUSED_K:
      # more results than one pass of the selection kernels holds: the paged search of BruteForce
      # needs the corpus resident (one scan per 1024 results), so the stream is ingested once
      # for this call -- rows in stream order, i.e. the reference's counter (:477-488)
      cached = BruteForce(k=self._k).index_from_dataset(self._candidates)
    if cached is not None:
      self._check_candidate_dim(cached._d, q)
      kk = min(k, cached._n)     # handle_incomplete_batches semantics: fewer rows than k (:465-468)
      scores, rows = cached._query_rows(q, kk, embedded=True)
      self._last_ids = cached._ids
      return scores, (rows + self._base_row if self._base_row else rows)
    lib = _lib.load()
    nq, d = q.shape
    # non-finite inputs: Streaming re-reads its dataset on every call, so the blocks are NOT validated (that would
    # double the traffic); the queries and the best score of every row are, without a synchronisation -- a violation
    # raises at the next call (see BruteForce.__init__ / include/tfrs_hip.h)
    if self._finite is None:
      self._finite = _IndexHandle()
    if self._finite.flags(reset=2) & 2:      # (set by a completed EARLIER call: the same deferred contract as BruteForce's)
      raise ValueError("Streaming: the queries or the best scores of an earlier call contained NaN or Inf; queries and "
                       "candidate blocks must be finite (include/tfrs_hip.h).")
    state_scores = torch.zeros((nq, k), dtype=torch.float32, device=q.device)
    state_rows = torch.zeros((nq, k), dtype=torch.int32, device=q.device)
    state_len = 0
    counter = self._base_row                                            # :421-422
    ids = []
    new_len = ctypes.c_int32(0)
    ws = None
    # Groups of consecutive blocks are searched where they lie (no packed copy) when the row
    # layout allows it: one launch chain per group instead of one per block.
    grouped = d in _RAW_DIMS and k <= MAX_FUSED_K
    group: list = []
    group_rows = 0
    group_base = counter

    def flush_group():
      nonlocal group, group_rows, group_base, state_len, ws
      if not group:
        return
      n = len(group)
      ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in group])
      rows = (ctypes.c_int64 * n)(*[b.shape[0] for b in group])
      need = lib.tfrs_streaming_topk_blocks_workspace_bytes(nq, group_rows, d, k)
      if ws is None or ws.numel() < need:
        ws = None
        ws = _workspace(need)
      _lib.check(lib.tfrs_streaming_topk_update_blocks(
          _lib.ptr(q), nq, d, ptrs, rows, n, group_base, group_base - self._base_row, k,
          _lib.ptr(state_scores), _lib.ptr(state_rows), state_len, ctypes.byref(new_len),
          _lib.ptr(ws), ws.numel(), _lib.current_stream()))            # :424-472 for every block of the group
      state_len = int(new_len.value)
      # The blocks are only referenced by the kernels just enqueued on THIS stream.  A block the dataset
      # produced on another stream would be handed back to that stream's allocator pool when the reference is
      # dropped, and could be overwritten before these kernels have read it: tell the allocator who reads it
      # (a no-op for blocks of the current stream).
      stream = torch.cuda.current_stream(q.device)
      for b in group:
        if b.is_cuda:
          b.record_stream(stream)
      group, group_rows = [], 0

    for block_ids, block in _iter_blocks(self._candidates):
      if block_ids is not None:
        # (device identifiers stay on the device: a `.cpu()` here would synchronise once per block)
        ids.append(block_ids if isinstance(block_ids, torch.Tensor) else np.asarray(block_ids))
      block = _as_f32_matrix(block, "candidates")
      nb = block.shape[0]
      self._check_candidate_dim(block.shape[1], q)
      if not self._handle_incomplete_batches and nb < k:               # :431-436, :34-54
        raise ValueError(BATCH_TOO_SMALL_MESSAGE.format(k=k))
      if counter + nb > _INT32_MAX:
        raise ValueError("Streaming: global row numbers exceed int32 (%d)" % (counter + nb))
      if d > MAX_FUSED_DIM:
        state_len = _wide_topk_update(q, block, counter, k, state_scores, state_rows, state_len)
        counter += nb
        continue
      if grouped and nb > 0 and block.data_ptr() % 16 == 0:
        if not group:
          group_base = counter
        group.append(block)
        group_rows += nb
        counter += nb
        if len(group) == _RAW_MAX_BLOCKS or group_rows * d * 4 >= self._group_bytes(q.device):
          flush_group()
        continue
      flush_group()          # (a block the grouped path cannot take: keep the stream order)
      need = lib.tfrs_streaming_topk_workspace_bytes(nq, nb, d, k)
      if ws is None or ws.numel() < need:
        ws = _workspace(need)
      _lib.check(lib.tfrs_streaming_topk_update(
          _lib.ptr(q), nq, d, _lib.ptr(block), nb, counter, k, _lib.ptr(state_scores),
          _lib.ptr(state_rows), state_len, ctypes.byref(new_len), _lib.ptr(ws),
          ws.numel(), _lib.current_stream()))                          # :424-472
      state_len = int(new_len.value)
      counter += nb                                                     # :477-478
    flush_group()
    all_ids = None
    if ids:
      if all(isinstance(i, torch.Tensor) for i in ids):
        # along axis 0 as the reference concatenates them (2-D identifier blocks keep their rows), on the
        # device of the first block (a mix of host and device blocks would make torch.cat raise)
        all_ids = torch.cat([i.to(ids[0].device) for i in ids], dim=0)
      else:
        all_ids = np.concatenate([i.cpu().numpy() if isinstance(i, torch.Tensor) else i for i in ids], axis=0)
    self._last_ids = _Identifiers(all_ids, counter - self._base_row)
    if state_len > 0 and nq > 0:
      # (the carried state with the queries in one launch; a state shorter than k -- fewer candidates than k -- is copied first)
      self._finite.note(q, state_scores[:, :state_len])
    return state_scores[:, :state_len], state_rows[:, :state_len]

  @staticmethod
  def _check_candidate_dim(d: int, q: Tensor) -> None:
    if d != q.shape[1]:
      raise ValueError(f"Candidate dimension {d} does not match queries ({q.shape[1]}).")

  def _group_bytes(self, device) -> int:
    if self._group_max_bytes is None:
      free = torch.cuda.mem_get_info(device)[0] if device.type == "cuda" else (8 << 30)
      self._group_max_bytes = max(64 << 20, min(8 << 30, free // 8))
    return self._group_max_bytes

  def _ids_of_rows(self, rows: Tensor):
    return self._last_ids.gather(rows - self._base_row if self._base_row else rows)

  def call(self, queries, k: Optional[int] = None):
    scores, rows = self._query_rows(queries, self._k_or_default(k))
    return scores, self._ids_of_rows(rows)                              # :438

  def is_exact(self) -> bool:
    return True
