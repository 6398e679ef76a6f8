"""Row-sharded top-K: one exchange, one merge (``ShardedBruteForce``, ``ShardedStreaming``)."""

import os
from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch

from recommenders_amd import _lib

from ._base import TopK
from ._common import _INT32_MAX, ArrayLike, Tensor, _check_identifier_rows, _Identifiers
from .brute_force import BruteForce
from .streaming import Streaming


_BASE_WORDS: dict = {}


def _base_row_words(base_row: int, dev) -> Tensor:
  """The two int32 words of a shard's int64 base row as a device tensor, built once per (device, base row):
  the wide exchange used to build them with ``torch.tensor([...])`` -- a host-to-device copy and a
  synchronisation point in every query."""
  key = (str(dev), int(base_row))
  words = _BASE_WORDS.get(key)
  if words is None:
    if len(_BASE_WORDS) > 64:
      _BASE_WORDS.clear()
    words = torch.tensor([base_row & 0xFFFFFFFF, base_row >> 32], dtype=torch.int64).to(torch.int32).to(dev)
    _BASE_WORDS[key] = words
  return words


def _pad_to_k(scores: Tensor, rows: Tensor, k: int) -> Tuple[Tensor, Tensor]:
  """A shard with fewer than ``k`` rows: pad its lists with empty slots (score -inf, row -1)."""
  pad = k - scores.shape[1]
  if pad <= 0:
    return scores, rows
  return (torch.cat([scores, scores.new_full((scores.shape[0], pad), float("-inf"))], dim=1),
          torch.cat([rows, rows.new_full((rows.shape[0], pad), -1)], dim=1))


def _exchange_and_merge_wide(scores: Tensor, local_rows: Tensor, k: int, group, merge: Optional[Callable],
                             base_row: int):
  """The same single exchange for corpora whose GLOBAL row numbers do not fit int32 ("ids
  beyond 2^31 need i64"; 8 x 288 GB of dim-64 rows are 9 * 10^9 rows; the reference's counter is int32,
  :380-382).  A shard always fits int32, so ranks exchange (score bits, LOCAL row) plus their int64 base
  row (two extra words of the same all_gather); the parts are ordered by base row and merged on the
  synthetic index ``part * k + position`` -- every part is already sorted (score desc, row asc), so part
  order then position IS global-row order among equal scores, and the 64-bit merge keys need no wider
  row field; ``base[part] + local[part, q, position]`` restores int64 global rows afterwards."""
  import torch.distributed as dist
  dev = scores.device
  nq = scores.shape[0]
  scores, local_rows = _pad_to_k(scores, local_rows, k)
  world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
  words = 2 * nq * k + 2
  mine = torch.empty((words,), dtype=torch.int32, device=dev)
  mine[:nq * k].copy_(scores.contiguous().view(torch.int32).reshape(-1))
  mine[nq * k:2 * nq * k].copy_(local_rows.to(torch.int32).reshape(-1))
  mine[2 * nq * k:].copy_(_base_row_words(base_row, dev))     # (device-resident: no host copy in the query path)
  gathered = torch.empty((world, words), dtype=torch.int32, device=dev)
  if world > 1 or os.environ.get("TFRS_FORCE_EXCHANGE", "0") == "1":
    dist.all_gather_into_tensor(gathered.view(-1), mine, group=group)
  else:
    gathered[0].copy_(mine)
  tail = gathered[:, 2 * nq * k:].to(torch.int64)
  bases = (tail[:, 0] & 0xFFFFFFFF) | (tail[:, 1] << 32)                  # [world] int64
  order = torch.argsort(bases)                                            # parts in global-row order
  parts = gathered.index_select(0, order)
  bases = bases.index_select(0, order)
  part_scores = parts[:, :nq * k].contiguous().view(torch.float32).reshape(world, nq, k)
  part_rows = parts[:, nq * k:2 * nq * k].reshape(world, nq, k)
  synth = (torch.arange(world, device=dev, dtype=torch.int32)[:, None, None] * k
           + torch.arange(k, device=dev, dtype=torch.int32)[None, None, :]).expand(world, nq, k)
  synth = torch.where(part_rows < 0, torch.full_like(part_rows, -1), synth).contiguous()
  if merge is not None:
    out_s, out_i = merge(part_scores, synth, k)
    out_s, out_i = out_s.to(dev), out_i.to(dev)
  else:
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, k), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tfrs_topk_merge(
        _lib.ptr(part_scores.contiguous()), _lib.ptr(synth), world, nq, k, k, _lib.ptr(out_s), _lib.ptr(out_i),
        None, 0, _lib.current_stream()))
  valid = out_i >= 0
  idx = out_i.clamp_min(0).long()
  part, pos = idx // k, idx % k
  qidx = torch.arange(nq, device=dev)[:, None].expand(nq, k)
  local = part_rows[part, qidx, pos].long()
  rows64 = torch.where(valid, bases[part] + local, torch.full_like(local, -1))
  return out_s, rows64


def _exchange_and_merge(scores: Tensor, rows: Tensor, k: int, group, merge: Optional[Callable]):
  """The ONE exchange step of row-sharded top-K: this rank's (score bits, global row)[nq, k]
  lists go back to back into one int32 buffer [2, nq, k]; a single all_gather delivers
  [world, 2, nq, k] (2 * nq * k * 4 bytes per rank, one direct xGMI send per peer) and the merge
  kernel reads the parts in place with the (score desc, row asc) rule, so every rank ends
  with exactly the single-GPU result."""
  import torch.distributed as dist
  if not (dist.is_available() and dist.is_initialized()):
    return scores, rows
  world = dist.get_world_size(group)
  if world == 1 and os.environ.get("TFRS_FORCE_EXCHANGE", "0") != "1":
    return scores, rows
  nq = scores.shape[0]
  scores, rows = _pad_to_k(scores, rows, k)
  mine = torch.empty((2, nq, k), dtype=torch.int32, device=scores.device)
  mine[0].copy_(scores.contiguous().view(torch.int32))
  mine[1].copy_(rows)
  gathered = torch.empty((world, 2, nq, k), dtype=torch.int32, device=scores.device)
  dist.all_gather_into_tensor(gathered.view(world * 2 * nq, k), mine.view(2 * nq, k), group=group)
  if merge is not None:
    return merge(gathered[:, 0].contiguous().view(torch.float32), gathered[:, 1].contiguous(), k)
  out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
  out_i = torch.empty((nq, k), dtype=torch.int32, device=scores.device)
  base = gathered.view(-1)
  _lib.check(_lib.load().tfrs_topk_merge_strided(
      base.data_ptr(), base.data_ptr() + nq * k * 4, world, 2 * nq * k, nq, k, k,
      _lib.ptr(out_s), _lib.ptr(out_i), _lib.current_stream()))
  return out_s, out_i


def _global_identifiers(rows: Tensor, local_ids: Optional[Tensor], base_row: int, n_local: int, group):
  """identifiers[global row] when every rank only holds the identifiers of its own rows: the
  owner fills its entries, one all_reduce(sum) of the [nq, k] int64 matrix completes it."""
  import torch.distributed as dist
  if local_ids is None:
    return rows
  local = rows.long() - base_row
  mine = (local >= 0) & (local < n_local)
  out = torch.zeros(rows.shape, dtype=torch.int64, device=rows.device)
  out[mine] = local_ids.to(rows.device).long()[local[mine]]
  if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
    dist.all_reduce(out, group=group)
  return out.to(local_ids.dtype)


def _check_shard_rows(base_row: int, n_local: int) -> None:
  if base_row < 0 or n_local > _INT32_MAX:
    raise ValueError(f"a shard holds at most 2^31 - 1 rows and base_row must be >= 0 (got {n_local} rows "
                     f"from row {base_row})")


def _any_rank_beyond_int32(base_row: int, n_local: int, group) -> bool:
  """True when some rank's global rows exceed int32 (decided once, at index time, with one small host
  collective, so that every rank takes the same exchange path): results are then int64 row numbers."""
  import torch.distributed as dist
  mine = base_row + n_local > _INT32_MAX
  if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
    return mine
  flags = [None] * dist.get_world_size(group)
  dist.all_gather_object(flags, bool(mine), group=group)
  return any(flags)


class ShardedBruteForce(TopK):
  """Brute-force retrieval over a corpus that is row-sharded across the GPUs of a node
  (one process per GPU, ``torch.distributed`` backend ``nccl`` = RCCL over xGMI).

  Rank r owns candidate rows ``[base_row, base_row + n_local)`` of the global corpus.
  ``call`` scores the (replicated) query batch against the local shard, all-gathers the
  per-shard ``(score, global row)[B, K]`` lists -- the only exchange step of the path,
  ``2 * B * K * 4`` bytes per rank -- and merges them with the same
  (score desc, row asc) rule, so every rank holds exactly the single-GPU result.
  ``identifiers`` (numeric, this shard's rows) are resolved by their owners and completed with
  one small all_reduce.  Not part of the reference (which has no multi-device top-K).
  """

  def __init__(self, query_model: Optional[Callable] = None, k: int = 10,
               process_group=None, name: Optional[str] = None,
               local_search: Optional[Callable] = None, merge: Optional[Callable] = None):
    super().__init__(k=k, name=name)
    self.query_model = query_model
    self._group = process_group
    self._local = BruteForce(k=k)
    self._base_row = 0
    self._n_local = 0
    self._local_ids: Optional[Tensor] = None
    self._ids = _Identifiers(None, 0)
    self._rows64 = False          # some rank's global rows exceed int32: exchange local rows + int64 bases
    self._cand = None             # the shard as given, for an injected `local_search`
    # injection points so the collective logic can be exercised on CPU (gloo) in tests
    self._local_search = local_search
    self._merge = merge

  def _set_shard(self, identifiers, n_local: int, base_row: int) -> None:
    """This rank's rows ``[base_row, base_row + n_local)`` and their identifiers (``None`` = global row numbers)."""
    _check_shard_rows(base_row, n_local)
    _check_identifier_rows(identifiers, n_local)
    if identifiers is not None and not isinstance(identifiers, torch.Tensor):
      identifiers = np.asarray(identifiers)
      if identifiers.dtype.kind not in "iub":
        raise NotImplementedError("ShardedBruteForce resolves integer identifiers only; map other "
                                  "identifier types from the returned global row numbers on the host.")
      identifiers = torch.as_tensor(identifiers)
    self._local_ids = identifiers
    self._base_row, self._n_local = base_row, n_local
    self._rows64 = _any_rank_beyond_int32(base_row, n_local, self._group)

  def index(self, candidates: ArrayLike, identifiers: Optional[ArrayLike] = None,
            base_row: int = 0) -> "ShardedBruteForce":
    self._set_shard(identifiers, len(candidates), int(base_row))
    if self._local_search is None:
      self._local.index(candidates)
    else:
      self._cand = candidates
    return self

  def index_from_dataset(self, candidates: Iterable, total_rows: Optional[int] = None,
                         base_row: int = 0) -> "ShardedBruteForce":
    """This rank's shard from an iterable of blocks (streamed into the device index when
    ``total_rows`` -- the shard's row count -- is given, see ``BruteForce.index_from_dataset``)."""
    self._local.index_from_dataset(candidates, total_rows=total_rows)
    ids = self._local._ids
    self._set_shard(ids.device if ids.device is not None else ids.host, self._local._n, int(base_row))
    return self

  def _query_rows(self, queries, k: int) -> Tuple[Tensor, Tensor]:
    if self._local_search is None:
      kk = min(k, self._local._n)
      scores, rows = self._local._query_rows(self._embed(queries), kk)
    else:
      scores, rows = self._local_search(queries, self._cand, k)
    if self._rows64:
      return _exchange_and_merge_wide(scores, rows, k, self._group, self._merge, self._base_row)
    rows = rows + self._base_row
    return _exchange_and_merge(scores, rows, k, self._group, self._merge)

  def call(self, queries, k: Optional[int] = None):
    scores, rows = self._query_rows(queries, self._k_or_default(k))
    return scores, _global_identifiers(rows, self._local_ids, self._base_row, self._n_local, self._group)

  def is_exact(self) -> bool:
    return True


class ShardedStreaming(Streaming):
  """``Streaming`` over a candidate stream that is row-sharded across ranks (BASELINE.json
  configs[2]: "Streaming top-100 sharded over 8 MI355X"): rank r streams ITS blocks, whose rows
  carry the global row numbers ``base_row, base_row + 1, ...``; the per-shard results are
  exchanged and merged exactly like ``ShardedBruteForce``.  Returns global row numbers
  (identifiers in the stream are resolved for the local rows only when every rank passes
  them; otherwise map rows on the host)."""

  def __init__(self, query_model: Optional[Callable] = None, k: int = 10,
               handle_incomplete_batches: bool = True, process_group=None,
               cache_packed_blocks: bool = True, merge: Optional[Callable] = None) -> None:
    super().__init__(query_model=query_model, k=k,
                     handle_incomplete_batches=handle_incomplete_batches,
                     cache_packed_blocks=cache_packed_blocks)
    self._group = process_group
    self._merge = merge
    self._rows64 = False          # the GLOBAL row count exceeds int32: stream with local rows, return int64 rows
    self._global_base = 0

  def index_from_dataset(self, candidates: Iterable, base_row: int = 0,
                         total_rows: Optional[int] = None) -> "ShardedStreaming":
    """``total_rows`` (the GLOBAL number of candidates, the same value on every rank): when it exceeds
    int32 the layer streams with shard-local row numbers and returns int64 global rows; without it a
    stream whose global rows pass 2^31 - 1 raises, as the int32 counter of the reference would wrap."""
    super().index_from_dataset(candidates)
    if base_row < 0:
      raise ValueError("base_row must be non-negative")
    self._rows64 = total_rows is not None and int(total_rows) > _INT32_MAX
    self._global_base = int(base_row)
    self._base_row = 0 if self._rows64 else int(base_row)
    return self

  def call(self, queries, k: Optional[int] = None):
    k = self._k_or_default(k)
    scores, rows = self._query_rows(queries, k)       # local shard; global row numbers unless rows64
    if self._rows64:
      return _exchange_and_merge_wide(scores, rows, k, self._group, self._merge, self._global_base)
    return _exchange_and_merge(scores, rows, k, self._group, self._merge)
