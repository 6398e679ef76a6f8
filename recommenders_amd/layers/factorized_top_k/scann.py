"""``ScaNN``: k-means tree, 4-bit product-quantized residuals, optional exact re-ordering."""

from typing import Any, Callable, Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from recommenders_amd import _lib

from ._base import TopK
from ._common import (MAX_FUSED_DIM, MAX_FUSED_K, NOT_INDEXED_MESSAGE, ArrayLike, Tensor, _as_f32_matrix,
                      _check_k_against_rows, _check_query_dim, _device, _Identifiers, _save_npz, _validate_candidates,
                      _workspace)
from .brute_force import BruteForce


_SCANN_SCORE_BUDGET_BYTES = 256 << 20   # bytes of the [B_chunk, P_max] f32 score buffer of one ScaNN search call
_SCANN_TRAIN_SAMPLE = 100000            # rows the tree and the codebooks are trained on
_SCANN_CODE_PAD = 128                   # zero code rows after the last leaf (the scan reads whole 128-row groups)
_SCANN_CHUNK_BYTES = 64 << 20           # temporaries of one index-time assignment chunk


def scann_probe_plan(leaf_sizes, num_leaves_to_search: int, k: int) -> Tuple[int, int]:
  """``(L_eff, P_max)`` of a ScaNN search: ``L_eff`` is the smallest ``L' >= num_leaves_to_search`` such that the
  ``L'`` SMALLEST leaves together hold at least ``k`` rows -- so every query's probed leaves hold ``k`` rows, whichever
  leaves it probes -- and ``P_max`` is the sum of the ``L_eff`` largest leaf sizes (the width of the score buffer).
  Host arithmetic on the leaf sizes, no device access."""
  sizes = np.sort(np.asarray(leaf_sizes, dtype=np.int64).reshape(-1))
  if sizes.size == 0 or k < 1 or int(sizes.sum()) < k:
    raise ValueError(f"input must have at least k columns (k={k}, candidates={int(sizes.sum())})")
  asc = np.concatenate([[0], np.cumsum(sizes)])
  desc = np.concatenate([[0], np.cumsum(sizes[::-1])])
  l_eff = max(max(1, min(int(num_leaves_to_search), sizes.size)), int(np.searchsorted(asc, k, side="left")))
  return l_eff, int(desc[l_eff])


def _first_distinct(x: np.ndarray, m: int) -> np.ndarray:
  """Positions of the first ``m`` distinct rows of ``x`` (bitwise), in order; fewer if ``x`` has fewer."""
  x = np.ascontiguousarray(x)
  for lim in (min(len(x), 64 * m), len(x)):
    rows = x[:lim].view(np.dtype((np.void, x.dtype.itemsize * x.shape[1]))).reshape(-1)
    _, first = np.unique(rows, return_index=True)
    if len(first) >= m or lim == len(x):
      return np.sort(first)[:m]
  return np.arange(0)


def _scann_nearest(x: Tensor, cent: Tensor) -> Tensor:
  """argmax_c x . mu_c - |mu_c|^2 / 2 (ties to the lower c) for x[n, dd], cent[m, dd]; or, blockwise, for x[n, nb, dd]
  and cent[nb, m, dd] (one argmax per block).  Chunked; f32, no atomics: the same inputs give the same answer."""
  half = 0.5 * (cent * cent).sum(-1)
  out = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
  per_row = max(1, int(np.prod(half.shape)))
  step = max(1, _SCANN_CHUNK_BYTES // (4 * per_row))
  for lo in range(0, x.shape[0], step):
    xs = x[lo:lo + step]
    if x.dim() == 2:
      s = xs @ cent.t() - half
    else:
      s = torch.einsum("sbd,bcd->sbc", xs, cent) - half
    out[lo:lo + step] = torch.argmax(s, dim=-1)
  return out


def _scann_lloyd(x_dev: Tensor, x_host: np.ndarray, cent: np.ndarray, iterations: int) -> np.ndarray:
  """Lloyd k-means under squared L2 from ``cent``: x[n, dd] against cent[m, dd], or blockwise x[n, nb, dd] against
  cent[nb, m, dd].  Means are float64 sums in row order (np.bincount), an empty cluster keeps its centre."""
  for _ in range(iterations):
    assign = _scann_nearest(x_dev, torch.as_tensor(cent, device=x_dev.device)).cpu().numpy()
    if x_host.ndim == 2:
      m = cent.shape[0]
      flat, vals = assign, x_host
    else:
      nb, m = cent.shape[0], cent.shape[1]
      flat = (assign + m * np.arange(nb)[None, :]).reshape(-1)
      vals = x_host.reshape(-1, x_host.shape[-1])
    size = m if x_host.ndim == 2 else nb * m
    counts = np.bincount(flat, minlength=size)
    sums = np.stack([np.bincount(flat, weights=vals[:, j], minlength=size) for j in range(vals.shape[1])], axis=1)
    prev = cent.reshape(size, -1)
    new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], prev).astype(np.float32)
    cent = new.reshape(cent.shape)
  return cent


def _pow2_exponent(maxabs: float) -> int:
  """e with maxabs * 2^e in [2^13, 2^14) (0 for 0): the fp16 scale of the scan (include/tfrs_hip.h)."""
  if not (maxabs > 0 and np.isfinite(maxabs)):
    return 0
  return 14 - int(np.frexp(np.float32(maxabs))[1])


class ScaNN(TopK):
  """ScaNN approximate retrieval (reference :613-796): a k-means tree over the candidates, 4-bit product-quantized
  residuals scanned on the matrix cores, and an optional exact re-ordering of the best candidates.

  ``index`` trains the index on the GPU (deterministic for a given ``seed``):
    * tree: Lloyd k-means (squared L2, ``training_iterations`` rounds) on a seeded sample of at most 100 000 rows,
      initialised from distinct sampled rows; every row goes to its nearest leaf centre;
    * rows are stable-sorted by leaf (leaf-major order);
    * codebooks: per block of ``dimensions_per_block`` dimensions (the last one may be partial), k-means with 16
      centres on the sampled residuals ``x - mu_leaf``, shared by all leaves; every row's residual is encoded as one
      4-bit code per block.
  ``call`` runs the leaf pass (exact ``BruteForce`` over the leaf centres), then one ``tfrs_scann_search`` per chunk
  of queries (csrc/scann.hip): decode + fp16 MFMA scan of the probed leaves, top ``max(k,
  num_reordering_candidates)`` of the approximate scores, exact f32 re-scoring of those when re-ordering is on, and
  the final top ``k`` under ``tf.math.top_k``'s order (score descending, lower row first).  No host synchronisation:
  ``make_graphed_call`` captures it.

  Deviations from the reference:
    * only ``distance_measure="dot_product"``; anything else raises ``NotImplementedError``;
    * ``parallelize_batch_searches`` is accepted and has no effect;
    * ``k`` and ``num_reordering_candidates`` are at most 1024 (``MAX_FUSED_K``) and ``d`` at most 128
      (``MAX_FUSED_DIM``); larger values raise ``ValueError``;
    * ``num_leaves`` is clipped to the row count, ``num_leaves_to_search`` to ``num_leaves``; a query probes more
      leaves than ``num_leaves_to_search`` when that many leaves could hold fewer than ``k`` rows;
    * the quantizer is plain product quantization, not ScaNN's anisotropic loss;
    * ``seed`` (not in the reference) seeds the training sample and its order (the initial leaf centres and codebook
      centres are the first distinct sampled rows), and therefore the whole index.
  """

  def __init__(self, query_model: Optional[Callable] = None, k: int = 10, distance_measure: str = "dot_product",
               num_leaves: int = 100, num_leaves_to_search: int = 10, training_iterations: int = 12,
               dimensions_per_block: int = 2, num_reordering_candidates: Optional[int] = None,
               parallelize_batch_searches: bool = True, name: Optional[str] = None, seed: int = 0):
    super().__init__(k=k, name=name)
    if distance_measure != "dot_product":
      raise NotImplementedError(f"ScaNN: distance_measure={distance_measure!r}; only 'dot_product' is implemented")
    if not 1 <= int(k) <= MAX_FUSED_K:
      raise ValueError(f"ScaNN: k={k} must be in [1, {MAX_FUSED_K}] (MAX_FUSED_K)")
    if int(num_leaves) < 1 or int(num_leaves_to_search) < 1:
      raise ValueError(f"ScaNN: num_leaves={num_leaves} and num_leaves_to_search={num_leaves_to_search} must be >= 1")
    if int(training_iterations) < 0:
      raise ValueError(f"ScaNN: training_iterations={training_iterations} must be >= 0")
    if int(dimensions_per_block) < 1:
      raise ValueError(f"ScaNN: dimensions_per_block={dimensions_per_block} must be >= 1")
    if num_reordering_candidates is not None and not 1 <= int(num_reordering_candidates) <= MAX_FUSED_K:
      raise ValueError(f"ScaNN: num_reordering_candidates={num_reordering_candidates} must be in [1, {MAX_FUSED_K}] "
                       "(MAX_FUSED_K)")
    self.query_model = query_model
    self._params = self._read_params(dict(
        num_leaves=num_leaves, num_leaves_to_search=num_leaves_to_search, training_iterations=training_iterations,
        dimensions_per_block=dimensions_per_block, num_reordering_candidates=num_reordering_candidates, seed=seed))
    self._parallelize_batch_searches = parallelize_batch_searches
    self._leaf_index: Optional[BruteForce] = None
    self._ids: Optional[_Identifiers] = None

  # -- index -------------------------------------------------------------------------------
  def index(self, candidates: ArrayLike, identifiers: Optional[ArrayLike] = None) -> "ScaNN":
    cand = _validate_candidates(candidates, identifiers)                # :712-722
    n, d = cand.shape
    if n < 1:
      raise ValueError("The candidates tensor is empty.")
    if d > MAX_FUSED_DIM:
      raise ValueError(f"ScaNN: embedding dim {d} above {MAX_FUSED_DIM} (MAX_FUSED_DIM)")
    if not bool(torch.isfinite(cand).all()):
      raise ValueError("The candidates contain NaN or Inf: ScaNN's k-means and codebooks need finite candidate rows. "
                       "Clean the embeddings before indexing them.")
    self._leaf_index = None                       # the previous index (if any) is dropped
    dev = cand.device
    rng = np.random.default_rng(self._params["seed"])
    # seeded random order: the distinct rows that start the tree and the codebooks are the first ones of this order,
    # not the corpus's lowest-numbered rows (item tables are often stored grouped by category or popularity)
    sample = rng.permutation(n)[:_SCANN_TRAIN_SAMPLE]
    xs = cand.index_select(0, torch.as_tensor(sample, device=dev))
    xs_host = xs.cpu().numpy()
    # tree
    num_leaves = min(self._params["num_leaves"], n)
    init = xs_host[_first_distinct(xs_host, num_leaves)]
    if init.shape[0] < num_leaves:                # fewer distinct rows than leaves: repeat the last one
      init = np.concatenate([init, np.repeat(init[-1:], num_leaves - init.shape[0], axis=0)])
    centroids = _scann_lloyd(xs, xs_host, init.astype(np.float32), self._params["training_iterations"])
    cent_dev = torch.as_tensor(centroids, device=dev)
    leaf = _scann_nearest(cand, cent_dev)
    leaf_sorted, perm = torch.sort(leaf, stable=True)
    counts = torch.bincount(leaf, minlength=num_leaves).cpu().numpy()
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    # codebooks on the sampled residuals
    dpb = min(self._params["dimensions_per_block"], d)
    nb = (d + dpb - 1) // dpb
    res_s = self._blocks(xs - cent_dev.index_select(0, _scann_nearest(xs, cent_dev)), nb, dpb)
    res_host = res_s.cpu().numpy()
    cb_init = np.zeros((nb, 16, dpb), dtype=np.float32)
    for b in range(nb):
      first = _first_distinct(res_host[:, b, :], 16)
      cb_init[b, :len(first)] = res_host[first, b, :]
      cb_init[b, len(first):] = res_host[first[-1], b, :]
    codebooks = _scann_lloyd(res_s, res_host, cb_init, self._params["training_iterations"])
    # codes of every row, leaf-major
    cb_dev = torch.as_tensor(codebooks, device=dev)
    code_bytes = ((nb + 1) // 2 + 3) // 4 * 4
    codes = torch.zeros((n, code_bytes), dtype=torch.uint8, device=dev)
    step = max(1, _SCANN_CHUNK_BYTES // (4 * (d + 16 * nb)))
    for lo in range(0, n, step):
      pos = perm[lo:lo + step]
      res = cand.index_select(0, pos) - cent_dev.index_select(0, leaf_sorted[lo:lo + step])
      c = _scann_nearest(self._blocks(res, nb, dpb), cb_dev).to(torch.uint8)
      if nb % 2:
        c = torch.cat([c, torch.zeros((c.shape[0], 1), dtype=torch.uint8, device=dev)], dim=1)
      codes[lo:lo + step, :c.shape[1] // 2] = c[:, 0::2] | (c[:, 1::2] << 4)
    rows = None
    if self._params["num_reordering_candidates"] is not None:
      rows = cand.index_select(0, perm)
    self._install(centroids, codebooks, codes, offsets, perm.to(torch.int32), rows, d)
    self._ids = _Identifiers(identifiers, n)
    return self

  @staticmethod
  def _blocks(x: Tensor, nb: int, dpb: int) -> Tensor:
    """x[n, d] -> [n, nb, dpb], the last block zero-padded."""
    pad = nb * dpb - x.shape[1]
    if pad:
      x = torch.cat([x, torch.zeros((x.shape[0], pad), dtype=x.dtype, device=x.device)], dim=1)
    return x.reshape(x.shape[0], nb, dpb).contiguous()

  def _install(self, centroids: np.ndarray, codebooks: np.ndarray, codes, offsets: np.ndarray, perm, rows,
               d: int) -> None:
    """Device image of a trained index (also the path of ``load_state_dict``: nothing is retrained)."""
    dev = _device()
    self._centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    self._codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    self._offsets_host = np.asarray(offsets, dtype=np.int64)
    self._sizes = np.diff(self._offsets_host)
    self._n, self._d = int(self._offsets_host[-1]), int(d)
    codes = torch.as_tensor(codes).to(dev, torch.uint8)
    self._codes = torch.cat([codes, torch.zeros((_SCANN_CODE_PAD, codes.shape[1]), dtype=torch.uint8,
                                                device=dev)]).contiguous()
    self._code_bytes = int(codes.shape[1])
    self._perm = torch.as_tensor(perm).to(dev, torch.int32).contiguous()
    self._rows = None if rows is None else torch.as_tensor(rows).to(dev, torch.float32).contiguous()
    self._offsets = torch.as_tensor(self._offsets_host, device=dev)
    nb, _, dpb = self._codebooks.shape
    self._lut_exp = _pow2_exponent(float(np.abs(self._codebooks).max(initial=0.0)))
    dp = (d + 15) // 16 * 16
    lut = np.zeros((dp, 16), dtype=np.float32)
    dims = np.arange(d)
    lut[:d] = np.ldexp(self._codebooks[dims // dpb, :, dims % dpb], self._lut_exp)
    self._lut = torch.as_tensor(lut.astype(np.float16), device=dev).contiguous()
    self._dpb_eff = int(dpb)
    self._leaf_index = BruteForce(k=1, dedup=False).index(self._centroids)

  # -- query -------------------------------------------------------------------------------
  def _check_indexed(self) -> None:
    if self._leaf_index is None:
      raise ValueError(NOT_INDEXED_MESSAGE)

  def probe_plan(self, k: Optional[int] = None) -> Tuple[int, int]:
    """``(L_eff, P_max)`` of a call with ``k`` results (``scann_probe_plan`` on the indexed leaf sizes)."""
    self._check_indexed()
    return scann_probe_plan(self._sizes, self._params["num_leaves_to_search"], self._k_or_default(k))

  def probe_leaves(self, queries, k: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The leaf pass of a call with ``k`` results: ``(scores [B, L_eff], leaves [B, L_eff])``, the exact top
    ``L_eff`` of ``q . mu`` over the leaf centres (score descending, lower leaf first) -- the leaves the call scans, in
    the order of its score buffer."""
    l_eff, _ = self.probe_plan(k)
    q = self._embed(queries)
    _check_query_dim(q, self._d)
    return self._leaf_index._query_rows(q, l_eff, embedded=True)

  def _query_rows(self, queries, k: int, embedded: bool = False) -> Tuple[Tensor, Tensor]:
    self._check_indexed()
    q = queries if embedded else self._embed(queries)
    _check_query_dim(q, self._d)
    _check_k_against_rows(k, self._n)
    if not 1 <= k <= MAX_FUSED_K:
      raise ValueError(f"ScaNN: k={k} must be in [1, {MAX_FUSED_K}] (MAX_FUSED_K)")
    r = max(k, self._params["num_reordering_candidates"] or k)
    l_eff, p_max = scann_probe_plan(self._sizes, self._params["num_leaves_to_search"], k)
    leaf_scores, probes = self._leaf_index._query_rows(q, l_eff, embedded=True)    # the leaf pass (probe_leaves)
    nq = q.shape[0]
    lib = _lib.load()
    out_s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    out_r = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    chunk = max(1, min(nq, _SCANN_SCORE_BUDGET_BYTES // (4 * p_max)))
    ws = _workspace(lib.tfrs_scann_search_workspace_bytes(chunk, len(self._sizes), l_eff, self._d, p_max, r))
    max_leaf = int(self._sizes.max())
    for lo in range(0, nq, chunk):
      hi = min(nq, lo + chunk)
      _lib.check(lib.tfrs_scann_search(
          _lib.ptr(q[lo:hi]), hi - lo, self._d, _lib.ptr(probes[lo:hi]), _lib.ptr(leaf_scores[lo:hi]), l_eff,
          _lib.ptr(self._offsets), len(self._sizes), max_leaf, _lib.ptr(self._codes), self._code_bytes,
          _lib.ptr(self._lut), self._dpb_eff, self._lut_exp, _lib.ptr(self._perm), _lib.ptr(self._rows), p_max, r, k,
          _lib.ptr(out_s[lo:hi]), _lib.ptr(out_r[lo:hi]), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    return out_s, out_r

  def _embed_any_rank(self, queries) -> Tuple[Tensor, bool]:
    """query_model, then rank 2 -> as is, rank 1 -> one query (:768-786); other ranks raise."""
    if self.query_model is not None:
      queries = self.query_model(queries)
    if not isinstance(queries, torch.Tensor):
      queries = torch.as_tensor(np.asarray(queries))
    if queries.dim() not in (1, 2):
      raise ValueError(f"Queries must be of rank 2 or 1, got {queries.dim()}.")
    single = queries.dim() == 1
    return _as_f32_matrix(queries.reshape(1, -1) if single else queries, "queries"), single

  def call(self, queries, k: Optional[int] = None):
    self._check_indexed()                                               # :757-761
    q, single = self._embed_any_rank(queries)
    scores, rows = self._query_rows(q, self._k_or_default(k), embedded=True)
    ids = self._ids.gather(rows)                                        # :788-791
    return (scores[0], ids[0]) if single else (scores, ids)

  def make_graphed_call(self, example_queries, k: Optional[int] = None):
    """``call`` for a fixed batch shape, captured once in a HIP graph and replayed (``TopK._graphed_call``, as
    ``BruteForce``'s): the leaf pass and every ``tfrs_scann_search`` launch are inside.  The layer must not be
    re-indexed afterwards."""
    self._check_indexed()
    return self._graphed_call(example_queries, self._k_or_default(k))

  def is_exact(self) -> bool:
    return False

  def index_bytes(self) -> int:
    """Device bytes held by the index: codes, row map, leaf offsets, code table, re-ordering rows, and the leaf
    centres' ``BruteForce`` (counted as f32 + fp16 images and a row map: 6 d + 4 bytes per leaf)."""
    self._check_indexed()
    ts = [self._codes, self._perm, self._offsets, self._lut] + ([self._rows] if self._rows is not None else [])
    return sum(t.numel() * t.element_size() for t in ts) + len(self._sizes) * (6 * self._d + 4)

  # -- persistence ---------------------------------------------------------------------------
  _PARAMS = ("num_leaves", "num_leaves_to_search", "training_iterations", "dimensions_per_block",
             "num_reordering_candidates", "seed")

  @classmethod
  def _read_params(cls, source: Mapping) -> Dict[str, Optional[int]]:
    """The ``_PARAMS`` of a mapping (constructor arguments, a state dict, the arrays of a saved file) as ints;
    ``num_reordering_candidates`` is ``None`` when absent, ``None`` or negative (a file stores -1)."""
    params = {p: int(source[p]) for p in cls._PARAMS if p != "num_reordering_candidates"}
    nrc = source.get("num_reordering_candidates")
    params["num_reordering_candidates"] = None if nrc is None or int(nrc) < 0 else int(nrc)
    return params

  def state_dict(self) -> Dict[str, Any]:   # type: ignore[override]
    """Everything that was trained (leaf centres, codebooks, codes, leaf offsets, row permutation, the leaf-major f32
    rows when re-ordering), the identifiers (``None`` = row numbers), ``k`` and the constructor parameters."""
    self._check_indexed()
    return {"centroids": self._centroids.copy(), "codebooks": self._codebooks.copy(),
            "codes": self._codes[:self._n].cpu().numpy(), "leaf_offsets": self._offsets_host.copy(),
            "perm": self._perm.cpu().numpy(), "rows": None if self._rows is None else self._rows.cpu().numpy(),
            "identifiers": self._ids.host_values(), "k": self._k, **self._params}

  def load_state_dict(self, state: Dict[str, Any]) -> "ScaNN":   # type: ignore[override]
    params = self._read_params(state)
    rows = state.get("rows")
    if (rows is None) != (params["num_reordering_candidates"] is None):
      raise ValueError("ScaNN state: the re-ordering rows must be present exactly when num_reordering_candidates is set")
    self._k = int(state.get("k", self._k))
    self._params = params
    centroids = np.asarray(state["centroids"], dtype=np.float32)
    self._install(centroids, state["codebooks"], np.asarray(state["codes"], dtype=np.uint8),
                  state["leaf_offsets"], np.asarray(state["perm"], dtype=np.int32), rows, centroids.shape[1])
    self._ids = _Identifiers(state.get("identifiers"), self._n)
    return self

  def save(self, path: str) -> None:
    """Writes the trained index to one ``.npz`` file; "no re-ordering" is stored as -1."""
    state = self.state_dict()
    if state["num_reordering_candidates"] is None:
      state["num_reordering_candidates"] = -1
    _save_npz(path, state)

  @classmethod
  def load(cls, path: str, query_model: Optional[Callable] = None) -> "ScaNN":
    with np.load(path, allow_pickle=False) as f:
      state = {key: f[key] for key in f.files}
    layer = cls(query_model=query_model, k=int(state["k"]), **cls._read_params(state))
    return layer.load_state_dict(state)
