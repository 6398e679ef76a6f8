"""What every top-K layer shares: device plumbing, messages, limits, the score / block helpers, the candidate-dataset
iterator, the identifier table, exclusions and the wrapper of the library's index handle."""

import ctypes
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from recommenders_amd import _lib

Tensor = torch.Tensor
ArrayLike = Union[torch.Tensor, np.ndarray, Sequence]

BATCH_TOO_SMALL_MESSAGE = (
    "Tried to retrieve k={k} top items, but the candidate "
    "dataset batch size is too small. This may be because "
    "your candidate batch size is too small or the last "
    "batch of your dataset is too small. "
    "To resolve this, increase your batch size, set the "
    "drop_remainder argument to True when batching your "
    "candidates, or set the handle_incomplete_batches "
    "argument to True in the constructor. ")

NOT_INDEXED_MESSAGE = ("The `index` method must be called first to "
                       "create the retrieval index.")


def _device() -> torch.device:
  if not torch.cuda.is_available():
    raise RuntimeError(
        "recommenders_amd needs a ROCm GPU (MI355X): no device is visible and "
        "there is no CPU fallback.")
  return torch.device("cuda", torch.cuda.current_device())


def _as_f32_matrix(x: ArrayLike, what: str) -> Tensor:
  """Float32, contiguous, 2-D, on the GPU."""
  if not isinstance(x, torch.Tensor):
    x = torch.as_tensor(np.asarray(x))
  if x.dim() != 2:
    raise ValueError(f"The {what} tensor must be 2D (got {tuple(x.shape)}).")
  return x.to(device=_device(), dtype=torch.float32).contiguous()


def _as_f32_queries(x: ArrayLike) -> Tensor:
  """Float32, contiguous, on the GPU: ``[B, D]`` queries or multi-head ``[B, H, D]`` queries (``BruteForce``)."""
  if not isinstance(x, torch.Tensor):
    x = torch.as_tensor(np.asarray(x))
  if x.dim() == 3:
    return x.to(device=_device(), dtype=torch.float32).contiguous()
  return _as_f32_matrix(x, "queries")


def _workspace(nbytes: int) -> Tensor:
  return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=_device())


_RAW_DIMS = (8, 16, 32, 64, 128)   # dims whose row-major rows the grouped Streaming path reads in place
_RAW_MAX_BLOCKS = 192              # blocks per tfrs_streaming_topk_update_blocks call (kRawMaxBlocks)
MAX_FUSED_DIM = 128    # TFRS_MAX_DIM: embedding dims the fused scan kernels keep in registers
MAX_FUSED_K = 1024     # TFRS_MAX_K: results per query the selection kernels hold in one pass
MAX_MERGE_HEADS = 32   # heads of a multi-head query (BruteForce on [B, H, D] queries)
MAX_MERGE_PAIRS = 8192  # heads * k (score, row) pairs one workgroup of tfrs_topk_merge_heads holds in LDS
_WIDE_BLOCK = 32768    # candidate rows per materialised score block on the wide-dim path

_INT32_MAX = 0x7FFFFFFF


def compute_scores(queries: Tensor, candidates: Tensor) -> Tensor:
  """``tf.matmul(queries, candidates, transpose_b=True)`` (``TopK._compute_score`` :320-333)
  through ``tfrs_compute_scores``: the candidate matrix is read in place (no transposed copy)."""
  from recommenders_amd.layers.feature_interaction import dcn
  q, c = queries.contiguous(), candidates.contiguous()
  nq, d = q.shape
  nc = c.shape[0]
  out = torch.empty((nq, nc), dtype=torch.float32, device=q.device)
  lib = _lib.load()
  f16 = 1 if dcn._use_f16_gemm(nq, nc, d) else 0
  ws = dcn._gemm_workspace(lib.tfrs_gemm_f16_workspace_bytes(nq, nc, d), q.device) if f16 else None
  _lib.check(lib.tfrs_compute_scores(_lib.ptr(q), _lib.ptr(c), nq, nc, d, _lib.ptr(out), f16,
                                     _lib.ptr(ws), ws.numel() if ws is not None else 0,
                                     _lib.current_stream()))
  return out


def _wide_topk_update(q: Tensor, block: Tensor, base_row: int, k: int, state_scores: Tensor,
                      state_rows: Tensor, state_len: int) -> int:
  """One candidate block of the wide-dim path (d > 128): materialised scores of at most
  ``_WIDE_BLOCK`` rows at a time, folded into the running state (:440-472)."""
  lib = _lib.load()
  new_len = ctypes.c_int32(state_len)
  for lo in range(0, block.shape[0], _WIDE_BLOCK):
    part = block[lo:lo + _WIDE_BLOCK]
    scores = compute_scores(q, part)
    _lib.check(lib.tfrs_topk_update_from_scores(
        _lib.ptr(scores), q.shape[0], part.shape[0], part.shape[0], base_row + lo, k,
        _lib.ptr(state_scores), _lib.ptr(state_rows), state_len, ctypes.byref(new_len),
        _lib.current_stream()))
    state_len = int(new_len.value)
  return state_len


def top_k_of_block(queries: Tensor, block: Tensor, k: int) -> Tuple[Tensor, Tensor]:
  """Exact top-``k`` (scores, row numbers) of ``queries @ block.T`` for ONE resident candidate block, with
  no index object, no host synchronisation and no ``[nq, n]`` matrix: the block is searched in place
  (``tfrs_streaming_topk_update_blocks``) when its layout allows it, else through the per-block entry
  point.  Used by ``tasks.Retrieval`` for hard-negative mining; capturable in a HIP graph."""
  q = queries.contiguous()
  block = block.contiguous()
  nq, d = q.shape
  n = block.shape[0]
  if not (1 <= k <= min(n, MAX_FUSED_K)) or d > MAX_FUSED_DIM:
    raise ValueError(f"top_k_of_block: k={k} / dim={d} outside the fused kernels' envelope")
  lib = _lib.load()
  scores = torch.zeros((nq, k), dtype=torch.float32, device=q.device)
  rows = torch.zeros((nq, k), dtype=torch.int32, device=q.device)
  new_len = ctypes.c_int32(0)
  if d in _RAW_DIMS and block.data_ptr() % 16 == 0:
    ws = _workspace(lib.tfrs_streaming_topk_blocks_workspace_bytes(nq, n, d, k))
    ptrs = (ctypes.c_void_p * 1)(block.data_ptr())
    counts = (ctypes.c_int64 * 1)(n)
    _lib.check(lib.tfrs_streaming_topk_update_blocks(
        _lib.ptr(q), nq, d, ptrs, counts, 1, 0, 0, k, _lib.ptr(scores), _lib.ptr(rows), 0,
        ctypes.byref(new_len), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
  else:
    ws = _workspace(lib.tfrs_streaming_topk_workspace_bytes(nq, n, d, k))
    _lib.check(lib.tfrs_streaming_topk_update(
        _lib.ptr(q), nq, d, _lib.ptr(block), n, 0, k, _lib.ptr(scores), _lib.ptr(rows), 0,
        ctypes.byref(new_len), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
  return scores, rows


def _check_candidates_with_identifiers(candidates: Iterable) -> None:
  """Precondition of the dataset used for indexing (reference :118-137), checked on
  the first element: either blocks, or 2-tuples with equal leading dimensions."""
  for first in candidates:
    if isinstance(first, (tuple, list)):
      if len(first) != 2:
        raise ValueError(
            "The dataset must yield candidate embeddings or "
            "tuples of (candidate identifiers, candidate embeddings). "
            f"Got a {len(first)}-tuple instead.")
      ids, cand = first
      if len(ids) != len(cand):
        raise ValueError(
            "Candidates and identifiers have to have the same batch dimension. "
            f"Got {len(cand)} and {len(ids)}.")
    break


def _iter_blocks(candidates: Iterable):
  """``(identifiers or None, block)`` of every element of a candidate dataset, both as the dataset gave them: no
  conversion, no device access."""
  for element in candidates:
    if isinstance(element, (tuple, list)):
      ids, block = element
      yield ids, block
    else:
      yield None, element


def _host_identifiers(ids) -> np.ndarray:
  return ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)


def _validate_candidates(candidates: ArrayLike, identifiers: Optional[ArrayLike]) -> Tensor:
  """The preconditions of ``index`` (reference :547-557, :712-722); returns the float32 device matrix."""
  if not isinstance(candidates, torch.Tensor):
    candidates = np.asarray(candidates)
  if candidates.ndim != 2:
    raise ValueError(f"The candidates tensor must be 2D (got {tuple(candidates.shape)}).")
  _check_identifier_rows(identifiers, candidates.shape[0])
  return _as_f32_matrix(candidates, "candidates")


def _check_identifier_rows(identifiers, nrows: int) -> None:
  if identifiers is not None and len(identifiers) != nrows:
    raise ValueError(
        "The candidates and identifiers tensors must have the same number of"
        f" rows (got {nrows} candidates rows and"
        f" {len(identifiers)} identifier rows). ")


def _check_query_dim(q: Tensor, d: int) -> None:
  if q.shape[1] != d:
    raise ValueError(f"Query dimension {q.shape[1]} does not match the index ({d}).")


def _check_k_against_rows(k: int, n: int) -> None:
  if k > n:
    raise ValueError(f"input must have at least k columns (k={k}, candidates={n})")


def _save_npz(path: str, state: Dict[str, Any]) -> None:
  """One ``.npz`` file of a layer's state: ``None`` entries are left out, string identifiers become a unicode array."""
  np.savez(path, **{key: np.asarray(val) for key, val in state.items() if val is not None})


class _Identifiers:
  """Identifier table: maps device row numbers to user identifiers (:607, :438) and
  user identifiers to comparable int32 codes for exclusions (:101-104)."""

  def __init__(self, values: Optional[ArrayLike], n: int):
    self.n = n
    self.host: Optional[np.ndarray] = None     # non-numeric identifiers
    self.device: Optional[Tensor] = None       # numeric identifiers
    self._code_of: Optional[Dict[Any, int]] = None
    self._codes_dev: Optional[Tensor] = None
    if values is None:
      return                                   # identifiers = arange(n), int32 (:544-545)
    if isinstance(values, torch.Tensor):
      self.device = values.to(_device())
    else:
      arr = np.asarray(values)
      if arr.dtype.kind in "iufb":
        self.device = torch.as_tensor(arr).to(_device())
      else:
        self.host = arr

  @property
  def is_range(self) -> bool:
    return self.host is None and self.device is None

  def host_values(self) -> Optional[np.ndarray]:
    """The identifiers as a host array (``None`` = row numbers), for checkpointing."""
    if self.host is not None:
      return self.host
    return None if self.device is None else self.device.cpu().numpy()

  def gather(self, idx: Tensor):
    """identifiers[idx] for an int32 index tensor."""
    if self.is_range:
      return idx
    if self.device is not None:
      return self.device[idx.long()]
    return self.host[idx.cpu().numpy()]

  def _build_codes(self) -> None:
    if self._code_of is not None:
      return
    vals = self.host if self.host is not None else self.device.cpu().numpy()
    uniq, inverse = np.unique(vals, return_inverse=True)
    self._uniq_host = uniq
    self._uniq_dev = (torch.as_tensor(uniq).to(_device())
                      if self.device is not None else None)
    self._code_of = {v.item() if hasattr(v, "item") else v: i for i, v in enumerate(uniq)}
    self._codes_dev = torch.as_tensor(inverse.astype(np.int32)).to(_device())

  def codes_of_rows(self, idx: Tensor) -> Tensor:
    """int32 code (rank among the distinct identifiers) of each retrieved row."""
    if self.is_range:
      return idx
    self._build_codes()
    return self._codes_dev[idx.long()].contiguous()

  def codes_of_values(self, values: ArrayLike) -> Tensor:
    """int32 codes of user-supplied identifiers (-1 = not in the index)."""
    if isinstance(values, torch.Tensor):
      values = values.cpu().numpy()
    arr = np.asarray(values)
    if self.is_range:
      codes = np.where((arr >= 0) & (arr < self.n), arr, -1).astype(np.int32)
    else:
      self._build_codes()
      flat = [self._code_of.get(v.item() if hasattr(v, "item") else v, -1)
              for v in arr.reshape(-1)]
      codes = np.asarray(flat, dtype=np.int32).reshape(arr.shape)
    return torch.as_tensor(codes).to(_device()).contiguous()

  def values_of_codes(self, codes: Tensor):
    if self.is_range:
      return codes
    if self._uniq_dev is not None:
      return self._uniq_dev[codes.long()]
    return self._uniq_host[codes.cpu().numpy()]


def _exclude(scores: Tensor, row_idx: Tensor, identifiers: _Identifiers,
             exclude: ArrayLike, k: int):
  """``_exclude`` (:83-115) through ``tfrs_topk_exclude``: candidates whose
  identifier is in the query's exclusion row are pushed down by 1e5, the top-k is
  re-taken, and the ORIGINAL scores / identifiers of the winners are returned.
  Identifiers are compared through int32 codes (rank among distinct identifiers)."""
  nq, kin = scores.shape
  codes = identifiers.codes_of_rows(row_idx).to(torch.int32).contiguous()
  excl = identifiers.codes_of_values(exclude)
  if excl.dim() != 2 or excl.shape[0] != nq:
    raise ValueError(
        f"exclusions must be [num_queries, num_to_exclude]; got {tuple(excl.shape)}")
  kout = min(k, kin)
  out_scores = torch.empty((nq, kout), dtype=torch.float32, device=scores.device)
  out_codes = torch.empty((nq, kout), dtype=torch.int32, device=scores.device)
  scores = scores.contiguous()
  _lib.check(_lib.load().tfrs_topk_exclude(
      _lib.ptr(scores), _lib.ptr(codes), nq, kin, _lib.ptr(excl), excl.shape[1], k,
      _lib.ptr(out_scores), _lib.ptr(out_codes), _lib.current_stream()))
  return out_scores, identifiers.values_of_codes(out_codes)


class _IndexHandle:
  """RAII wrapper of ``tfrs_index_t``: the packed device index of ``BruteForce`` and, left empty, the deferred
  finiteness record of the searches that have no index (``Streaming`` over blocks read in place)."""

  def __init__(self):
    self.handle = ctypes.c_void_p()
    self._lib = _lib.load()
    _lib.check(self._lib.tfrs_index_create(ctypes.byref(self.handle)))

  def __del__(self):
    h, self.handle = self.handle, None
    if h:
      try:
        self._lib.tfrs_index_destroy(h)
      except Exception:  # interpreter shutdown
        pass

  def flags(self, reset: int = 0) -> int:
    """The host-visible flag word (``tfrs_index_nonfinite``): bit 0 non-finite candidates, bit 1 non-finite queries
    of a call whose kernels have completed; the bits of ``reset`` are cleared.  Reading it does not synchronise."""
    out = ctypes.c_int32(0)
    _lib.check(self._lib.tfrs_index_nonfinite(self.handle, int(reset), ctypes.byref(out)))
    return int(out.value)

  def note(self, *tensors: Tensor) -> None:
    """ORs "some element is NaN / Inf" into bit 1 of the flag word -- ONE tiny launch per two tensors, no
    synchronisation (``tfrs_index_note_nonfinite``; the first version of this record was ten torch kernels, 50 us of a
    1.4 ms single-query call)."""
    if torch.cuda.is_current_stream_capturing():
      return                     # (a replayed graph runs no host code: nothing could read the flag)
    flat = [t.contiguous() for t in tensors if t.numel() > 0]
    for i in range(0, len(flat), 2):
      x, y = flat[i], (flat[i + 1] if i + 1 < len(flat) else None)
      _lib.check(self._lib.tfrs_index_note_nonfinite(
          self.handle, _lib.ptr(x), x.numel(), _lib.ptr(y), y.numel() if y is not None else 0, 2,
          _lib.current_stream()))
