"""``ClippyAdagrad``: Adagrad with adaptive clipping (``experimental/optimizers/clippy_adagrad.py``,
https://arxiv.org/abs/2302.09178) on MI355X.

Per variable and step (``update_step``, ``:188-254``), with ``acc`` the Adagrad accumulator::

    [use_standard_accumulator_update:  acc += g * g  first]
    pre    = 1 / sqrt(acc + epsilon)
    delta  = learning_rate * g * pre
    maxd   = |w| * variable_relative_threshold + pre * accumulator_relative_threshold + absolute_threshold
    factor = min(1, min_i (delta_i == 0 ? 1 : maxd_i / |delta_i|))          (``shrink_by_references``, ``:21-70``)
    w     -= delta * factor
    [otherwise:  acc += (clip_accumulator_update ? g * factor : g)^2  after]

so no element of ``w`` moves by more than ``maxd``.  The factor is a min over the whole variable -- for the
``(ids, rows)`` slices of an embedding lookup over the touched rows, after duplicates are summed -- and must be known
before anything is written: float32 parameters on the GPU go through the two-pass kernels ``tfrs_clippy_dense_multi``
(up to 32 tensors per call) and ``tfrs_clippy_sparse``; the factor stays on the device, so a step has no host
synchronisation and can be captured in a HIP graph.  Anything else (CPU tensors, float64) takes the same formula in
torch ops.

``learning_rate`` is a float, a ``recommenders_amd.schedules.LearningRateSchedule`` (the reference's
``Union[float, LearningRateSchedule]``, ``:96-113``), a 0-d float32 device tensor or a zero-argument callable returning
one: anything but a float is read by both kernel passes from a device float that ``tfrs_lr_tick`` writes at the head of
the step from the device counter ``iterations``, so a captured step replays the schedule (``optimizers`` module
docstring).  With a float there is no counter (``iterations`` is ``None``; a host counter would be frozen
by graph replay).

Deviations from the reference: row-sharded tables raise ``NotImplementedError`` (their factor would need a
min across ranks).
"""

import ctypes
from typing import Iterable, List, Sequence, Tuple

import torch

from recommenders_amd import optimizers as _base
from recommenders_amd.layers import embedding as emb


def shrink_by_references(tensor: torch.Tensor, references: Sequence[torch.Tensor],
                         relative_factors: Sequence[float],
                         absolute_factor: float) -> Tuple[torch.Tensor, torch.Tensor]:
  """Scales ``tensor`` by the largest ``0 <= scale <= 1`` such that for every element
  ``|tensor_i| * scale <= sum_j |reference_j_i| * relative_factor_j + absolute_factor``; returns
  ``(tensor * scale, scale)``.  ``references`` broadcast against ``tensor``."""
  if any(relative_factor < 0 for relative_factor in relative_factors):
    raise ValueError("relative_factors must all be non-negative.")
  if absolute_factor < 0:
    raise ValueError("absolute_factor must be non-negative.")
  if len(references) != len(relative_factors):
    raise ValueError(
        "references and relative_factors must have the same length. "
        f"Instead they are {len(references)} and {len(relative_factors)}.")
  max_delta = torch.full((), absolute_factor, dtype=tensor.dtype, device=tensor.device)
  for reference, relative_factor in zip(references, relative_factors):
    max_delta = max_delta + torch.abs(reference) * relative_factor
  # both tensor_i and max_delta_i may be zero: a zero max_delta forces scale 0, a zero tensor_i leaves it free
  per_element_scale = torch.where(tensor == 0, torch.ones_like(tensor), max_delta / torch.abs(tensor))
  one = torch.ones((), dtype=tensor.dtype, device=tensor.device)
  scale = torch.minimum(one, per_element_scale.min()) if per_element_scale.numel() else one
  return tensor * scale, scale


def _mode(group) -> int:
  return 2 if group["use_standard_accumulator_update"] else (1 if group["clip_accumulator_update"] else 0)


def clippy_update(w: torch.Tensor, acc: torch.Tensor, g: torch.Tensor, group) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """The formula of the module docstring in torch ops: ``(new w, new acc, factor)`` for same-shaped ``w, acc, g``."""
  mode = _mode(group)
  if mode == 2:
    acc = acc + g * g
  pre = 1.0 / torch.sqrt(acc + group["epsilon"])
  delta = group["learning_rate"] * g * pre
  clipped, factor = shrink_by_references(
      delta, [w, pre], [group["variable_relative_threshold"], group["accumulator_relative_threshold"]],
      group["absolute_threshold"])
  if mode != 2:
    update = g * factor if mode == 1 else g
    acc = acc + update * update
  return w - clipped, acc, factor


class ClippyAdagrad(_base.SliceOwningOptimizer):
  """``tfrs.experimental.optimizers.ClippyAdagrad``.  ``clipping_factors`` (with ``export_clipping_factors``) is a
  list of 0-d device tensors in parameter order, views of one buffer that every step updates in place."""

  _CONFIG = ("learning_rate", "initial_accumulator_value", "variable_relative_threshold",
             "accumulator_relative_threshold", "absolute_threshold", "epsilon", "export_clipping_factors",
             "clip_accumulator_update", "use_standard_accumulator_update")

  def __init__(self, params: Iterable, learning_rate=0.001, initial_accumulator_value: float = 0.1,
               variable_relative_threshold: float = 0.1, accumulator_relative_threshold: float = 0.0,
               absolute_threshold: float = 1e-7, epsilon: float = 1e-7, export_clipping_factors: bool = False,
               clip_accumulator_update: bool = False, use_standard_accumulator_update: bool = False):
    if clip_accumulator_update and use_standard_accumulator_update:
      raise ValueError("clip_accumulator_update and use_standard_accumulator_update cannot both be set to True.")
    if variable_relative_threshold < 0 or accumulator_relative_threshold < 0 or absolute_threshold < 0:
      raise ValueError("the clipping thresholds must be non-negative")
    super().__init__(params, dict(
        learning_rate=learning_rate, initial_accumulator_value=float(initial_accumulator_value),
        variable_relative_threshold=float(variable_relative_threshold),
        accumulator_relative_threshold=float(accumulator_relative_threshold),
        absolute_threshold=float(absolute_threshold), epsilon=float(epsilon),
        export_clipping_factors=bool(export_clipping_factors), clip_accumulator_update=bool(clip_accumulator_update),
        use_standard_accumulator_update=bool(use_standard_accumulator_update)))
    all_params = [p for group in self.param_groups for p in group["params"]]
    for p in all_params:
      if getattr(p, "_tfrs_row_sharded", False):
        self.close()
        raise NotImplementedError("ClippyAdagrad on a row-sharded table: its clipping factor would need a min "
                                  "across ranks")
    if len({p.device for p in all_params}) > 1:
      self.close()
      raise ValueError("ClippyAdagrad: all parameters must live on one device (the clipping factors are one device "
                       "buffer that the kernels write); build one ClippyAdagrad per device")
    self._index = {p: i for i, p in enumerate(all_params)}
    device = all_params[0].device if all_params else torch.device("cpu")
    # one slot per parameter: the kernels write a parameter's factor into its slot (and read it back in the apply
    # pass), whether it is exported or not
    self._factors = torch.ones((max(len(all_params), 1),), dtype=torch.float32, device=device)
    self.clipping_factors: List[torch.Tensor] = (
        [self._factors[i] for i in range(len(all_params))] if export_clipping_factors else [])
    self._init_learning_rate()

  def _hyper(self, group) -> Tuple[float, float, float, float, float, int]:
    return (self._step_lr(group), group["epsilon"], group["variable_relative_threshold"],
            group["accumulator_relative_threshold"], group["absolute_threshold"], _mode(group))

  def _dense_call(self, items, first_slot: int, group) -> None:
    """``items``: (parameter, accumulator, gradient) of consecutive factor slots starting at ``first_slot``."""
    from recommenders_amd import _lib
    n = len(items)
    vp, i64a = ctypes.c_void_p * n, ctypes.c_int64 * n
    (lr, lr_dev), eps, var_rel, acc_rel, abs_thr, mode = self._hyper(group)
    args = (n, vp(*[p.data_ptr() for p, _, _ in items]), vp(*[a.data_ptr() for _, a, _ in items]),
            vp(*[g.data_ptr() for _, _, g in items]), i64a(*[p.numel() for p, _, _ in items]),
            ctypes.c_void_p(self._factors.data_ptr() + 4 * first_slot), lr)
    _lib.check(_lib.load().tfrs_clippy_dense_multi_dlr(*args, _lib.ptr(lr_dev), eps, var_rel, acc_rel, abs_thr, mode,
                                                       _lib.current_stream()))
    self._wrote(*[p for p, _, _ in items])

  def _sparse_call(self, p, acc, ids, rows, group) -> None:
    from recommenders_amd import _lib
    lib = _lib.load()
    d = p.shape[1]
    flat, g = emb._flat_slices(ids, rows, d)
    n = flat.numel()
    rowscan = 1 if emb._use_rowscan(p.shape[0], n, d) else 0
    ws = torch.empty((lib.tfrs_clippy_sparse_workspace_bytes(n, rowscan),), dtype=torch.uint8, device=p.device)
    (lr, lr_dev), eps, var_rel, acc_rel, abs_thr, mode = self._hyper(group)
    _lib.check(lib.tfrs_clippy_sparse_dlr(
        _lib.ptr(g), _lib.ptr(flat), 1 if flat.dtype == torch.int64 else 0, n, d, p.shape[0], _lib.ptr(p.data),
        _lib.ptr(acc), ctypes.c_void_p(self._factors.data_ptr() + 4 * self._index[p]), lr, _lib.ptr(lr_dev), eps,
        var_rel, acc_rel, abs_thr, mode, rowscan, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    self._wrote(p)

  def _sparse_fallback(self, p, acc, ids, rows, group) -> None:
    uniq, summed = self._summed_slices(p, ids, rows, rows.dtype)     # (the gradient's own precision, like the kernels)
    w, a, factor = clippy_update(p.data[uniq], acc[uniq], summed.to(p.dtype), group)
    p.data[uniq] = w
    acc[uniq] = a
    self._factors[self._index[p]].copy_(factor)

  @torch.no_grad()
  def step(self, closure=None):
    loss = self._closure_loss(closure)
    self._tick()
    for group in self.param_groups:
      init = group["initial_accumulator_value"]
      for p in group["params"]:
        merged = self._merged_slices(p)
        if merged is None:
          continue
        ids, rows = merged
        acc = self._accumulator(p, init)
        if self._on_kernel_route(p, [acc], rows) and ids.device == p.device:
          self._sparse_call(p, acc, ids, rows, group)
        else:
          self._sparse_fallback(p, acc, ids.to(p.device), rows.to(p.device), self._host_group(group))
      run: List[tuple] = []     # dense parameters of consecutive factor slots: one call per 32
      first = 0
      for p in group["params"]:
        acc = self._accumulator(p, init)
        if p.grad is None:
          continue
        g, slot = p.grad, self._index[p]
        if self._on_kernel_route(p, [acc], g):
          if run and (slot != first + len(run) or len(run) == 32):
            self._dense_call(run, first, group)
            run = []
          if not run:
            first = slot
          run.append((p, acc, g.contiguous()))
          continue
        w, a, factor = clippy_update(p.data, acc, g.to_dense() if g.is_sparse else g, self._host_group(group))
        p.data.copy_(w)
        acc.copy_(a)
        self._factors[slot].copy_(factor)
      if run:
        self._dense_call(run, first, group)
    return loss
