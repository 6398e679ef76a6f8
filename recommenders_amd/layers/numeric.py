"""Numeric preprocessing layers: ``Discretization`` and ``Normalization`` on the kernels of ``csrc/numeric.hip``.

The reference's tutorials (``featurization``, ``context_features``, ``deep_recommenders``) build the timestamp half of
the user tower from ``tf.keras.layers.Discretization(timestamp_buckets)`` in front of an ``Embedding`` and
``tf.keras.layers.Normalization(axis=None)``.  Keras is not part of the reference tree, so the rules below are the
contract of these layers.

``Discretization`` maps a value to the number of boundaries ``<=`` it (``np.searchsorted(side="right")``) the way
TensorFlow's ``Bucketize`` kernel does: the boundaries are 32-bit floats; f32 input is compared in f32, int32 and int64
input is first rounded to f32 (to nearest even), f64 input is compared in f64 against the widened boundaries; NaN goes
to the last bucket.  An int64 unix timestamp that is no f32 value can therefore land one bucket away from where an f64
comparison would put it -- as it does in TensorFlow.  ``adapt`` with ``num_bins`` takes EXACT quantiles (one sort),
where Keras sketches them with rank error ``epsilon``.

``Normalization`` converts its input to f32 and returns ``(x - mean) / max(sqrt(variance), 1e-7)``, an IEEE
subtraction and an IEEE division, or with ``invert=True`` ``fma(x, scale, mean)``.  ``adapt`` accumulates the mean and
the population variance of the f32 values in f64 on the device (per workgroup, then merged pairwise in a fixed order:
the same bits on every run) and rounds them to f32 once.

Both forwards launch one kernel, allocate nothing but their output and never synchronise, so they can sit inside a
captured step; so can ``Normalization.update_state`` (two launches on a workspace that is allocated once).
"""

from typing import Optional

import numpy as np
import torch

from recommenders_amd import _lib
from recommenders_amd.layers.hashing import _device
from recommenders_amd.layers.preprocessing import _batches, _values_of

LDS_BOUNDARIES = 4095          # TFRS_BUCKETIZE_LDS_BOUNDARIES: more boundaries are searched in global memory
EPSILON = 1e-7                 # TFRS_NORMALIZE_EPSILON: Keras' backend.epsilon()
MOMENTS_SLICE_ELEMENTS = 4096  # TFRS_MOMENTS_SLICE_ELEMENTS: elements one workgroup of the moments pass reduces
MOMENTS_MAX_GROUPS = 1024      # TFRS_MOMENTS_MAX_GROUPS: workgroups of that pass; the slices grow beyond
_FORWARD, _INVERT, _BACKWARD = 0, 1, 2    # TFRS_NORMALIZE_*
_DTYPE_CODES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}   # TFRS_NUMERIC_*


def _as_numeric(inputs, dev: Optional[torch.device]) -> torch.Tensor:
  """A tensor, array or list -> a contiguous f32 / f64 / int32 / int64 tensor (on ``dev`` when given).  Narrower
  floats widen to f32 and narrower integers to int32, both exactly; bool, complex and strings raise ``ValueError``."""
  if not isinstance(inputs, torch.Tensor):
    arr = np.asarray(inputs)
    if arr.dtype.kind not in ("f", "i", "u"):
      raise ValueError(f"numeric input needed; got dtype {arr.dtype}")
    if arr.dtype.kind == "u":
      arr = arr.astype(np.int64 if arr.dtype.itemsize >= 4 else np.int32)
    elif arr.dtype == np.float16:
      arr = arr.astype(np.float32)
    inputs = torch.from_numpy(np.ascontiguousarray(arr))
  t = inputs.detach() if not inputs.requires_grad else inputs
  if t.dtype not in _DTYPE_CODES:
    if t.dtype in (torch.float16, torch.bfloat16):
      t = t.float()
    elif t.dtype in (torch.int8, torch.int16, torch.uint8):
      t = t.int()
    else:
      raise ValueError(f"numeric input needed (f32, f64, int32 or int64); got {t.dtype}")
  if dev is not None:
    t = t.to(dev)
  return t.contiguous()


# ---- Discretization --------------------------------------------------------------------------------------------------
def _check_boundaries(bin_boundaries) -> np.ndarray:
  """-> f32 boundaries; ``ValueError`` unless they are non-decreasing (repeats are legal) and free of NaN, judged on
  the f32 values the kernel compares against."""
  if isinstance(bin_boundaries, torch.Tensor):
    bin_boundaries = bin_boundaries.detach().cpu().numpy()
  arr = np.asarray(bin_boundaries if len(bin_boundaries) else [], dtype=np.float64).reshape(-1)
  with np.errstate(over="ignore"):
    b = arr.astype(np.float32)
  if np.isnan(b).any():
    raise ValueError("`bin_boundaries` must not contain NaN")
  if b.size > 1 and bool((b[1:] < b[:-1]).any()):
    raise ValueError("`bin_boundaries` must be sorted (non-decreasing)")
  return b


class Discretization(torch.nn.Module):
  """``tf.keras.layers.Discretization``: values of any shape -> int64 bucket indices of that shape on the GPU.

  ``Discretization(bin_boundaries=[b0, b1, ...])``: bucket ``i`` is ``[b_{i-1}, b_i)``, so a value equal to a boundary
  belongs to the bucket above it and there are ``len(bin_boundaries) + 1`` buckets -- the size of the ``Embedding``
  behind it.  ``Discretization(num_bins=k)`` learns ``k - 1`` boundaries in ``adapt(data)``: boundary ``i`` is the
  smallest value with at least ``i n / k`` of the ``n`` values at or below it (``np.quantile(method="inverted_cdf")``
  of the f32 values).  These quantiles are exact; ``epsilon``, the rank error of Keras' sketch, is accepted and
  ignored.

  The boundaries are an f32 buffer on the device and part of ``state_dict()``."""

  def __init__(self, bin_boundaries=None, num_bins: Optional[int] = None, epsilon: float = 0.01,
               output_mode: str = "int", sparse: bool = False, device: Optional[torch.device] = None):
    super().__init__()
    if output_mode != "int":
      raise NotImplementedError(f"output_mode={output_mode!r}: only 'int' is on the hot path")
    if sparse:
      raise NotImplementedError("sparse=True belongs to the one_hot / multi_hot / count outputs, which are not built")
    if bin_boundaries is not None and num_bins is not None:
      raise ValueError("pass `bin_boundaries` or `num_bins`, not both")
    if bin_boundaries is None and num_bins is None:
      raise ValueError("one of `bin_boundaries` and `num_bins` is needed")
    if num_bins is not None and int(num_bins) < 1:
      raise ValueError(f"`num_bins` must be at least 1; got {num_bins}")
    self.num_bins = None if num_bins is None else int(num_bins)
    self.epsilon = float(epsilon)
    self.output_mode = output_mode
    self.sparse = False
    self._device = device
    self.register_buffer("bin_boundaries", None)
    if bin_boundaries is not None:
      self._set_boundaries(_check_boundaries(bin_boundaries))

  def _set_boundaries(self, b) -> None:
    if isinstance(b, np.ndarray):
      b = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32))
    self.bin_boundaries = b.to(_device(self._device)).contiguous()

  def adapt(self, data) -> None:
    """Learns ``num_bins - 1`` boundaries: ``data`` is a tensor, an array or an iterable of batches."""
    if self.num_bins is None:
      raise RuntimeError("`adapt` needs `num_bins`; this layer was built from `bin_boundaries`")
    dev = _device(self._device)
    values = [_as_numeric(_values_of(batch), dev).reshape(-1).float() for batch in _batches(data)]
    values = torch.cat(values) if values else torch.empty((0,), dtype=torch.float32, device=dev)
    if bool(torch.isnan(values).any()):
      raise ValueError("`adapt` data must not contain NaN")
    n = values.numel()
    if n == 0:
      raise ValueError("`adapt` needs at least one value")
    ordered = torch.sort(values).values
    i = torch.arange(1, self.num_bins, dtype=torch.int64, device=dev)
    rank = (i * n + self.num_bins - 1) // self.num_bins          # ceil(i n / num_bins) values are <= the boundary
    self._set_boundaries(ordered[(rank - 1).clamp_(0, n - 1)])

  def forward(self, inputs) -> torch.Tensor:
    if self.bin_boundaries is None:
      if self.num_bins is not None:
        raise RuntimeError("call `adapt(data)` before the layer: `num_bins` is set and no boundaries are learned yet")
      self._set_boundaries(np.empty((0,), np.float32))
    b = self.bin_boundaries
    if not b.is_cuda:
      raise RuntimeError("recommenders_amd ops need a GPU; there is no CPU fallback.")
    x = _as_numeric(inputs, b.device)
    out = torch.empty(x.shape, dtype=torch.int64, device=b.device)
    _lib.check(_lib.load().tfrs_bucketize(_lib.ptr(x), _DTYPE_CODES[x.dtype], x.numel(), _lib.ptr(b), b.numel(),
                                          _lib.ptr(out), _lib.current_stream()))
    return out

  def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
    loaded = state_dict.get(prefix + "bin_boundaries")
    if loaded is not None:          # the number of boundaries is part of the state: make room for it
      self._set_boundaries(torch.empty(loaded.shape, dtype=torch.float32))
    super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


# ---- Normalization ---------------------------------------------------------------------------------------------------
def _launch_normalize(x: torch.Tensor, mean: torch.Tensor, scale: torch.Tensor, mode: int) -> torch.Tensor:
  f = mean.numel()
  out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
  _lib.check(_lib.load().tfrs_normalize(_lib.ptr(x), _DTYPE_CODES[x.dtype], x.numel() // f, f, _lib.ptr(mean),
                                        _lib.ptr(scale), mode, _lib.ptr(out), _lib.current_stream()))
  return out


class _Normalize(torch.autograd.Function):
  """One launch forward, one launch backward (the gradient of the input; the statistics are constants)."""

  @staticmethod
  def forward(ctx, x, mean, scale, invert):
    ctx.save_for_backward(mean, scale)
    ctx.invert = invert
    ctx.in_dtype = x.dtype
    return _launch_normalize(x, mean, scale, _INVERT if invert else _FORWARD)

  @staticmethod
  def backward(ctx, grad):
    mean, scale = ctx.saved_tensors
    dx = _launch_normalize(grad.float().contiguous(), mean, scale, _BACKWARD | (_INVERT if ctx.invert else 0))
    return dx.to(ctx.in_dtype), None, None, None


class Normalization(torch.nn.Module):
  """``tf.keras.layers.Normalization``: ``(x - mean) / max(sqrt(variance), 1e-7)`` in f32 on the GPU.

  ``axis=None``: one mean and one variance over everything (the tutorials' timestamp).  ``axis=-1`` (default): one per
  feature of the last axis.  The statistics come from ``mean=`` and ``variance=`` (which broadcast to the feature
  shape) or from ``adapt(data)`` = ``reset_state()``, ``update_state(batch)`` per batch, ``finalize_state()``.
  ``mean``, ``variance`` (f32) and ``count`` (int64) are buffers, as is the f64 running state ``moments[f, 3]``
  (count, mean, sum of squared deviations), so an interrupted ``adapt`` resumes from a ``state_dict()``.
  ``invert=True`` maps normalised values back: ``x * scale + mean``, fused.

  The output is f32 of the input's shape; the gradient reaches a floating-point input through one more launch."""

  def __init__(self, axis=-1, mean=None, variance=None, invert: bool = False,
               device: Optional[torch.device] = None):
    super().__init__()
    if isinstance(axis, (tuple, list)):
      axis = axis[0] if len(axis) == 1 else tuple(axis)
    if axis is not None and axis != -1:
      raise NotImplementedError(f"axis={axis!r}: only axis=None and axis=-1 are on the hot path")
    if (mean is None) != (variance is None):
      raise ValueError("`mean` and `variance` must be given together (or neither, for `adapt`)")
    self.axis = axis
    self.invert = bool(invert)
    self._device = device
    self._workspace = None
    for name in ("mean", "variance", "count", "moments"):
      self.register_buffer(name, None)
    self.register_buffer("_scale", None, persistent=False)
    self._ready = False
    self._given_scalar = False      # scalar `mean` / `variance` under axis=-1 broadcast over any last axis
    if mean is not None:
      m = np.asarray(mean.detach().cpu() if isinstance(mean, torch.Tensor) else mean, dtype=np.float32)
      v = np.asarray(variance.detach().cpu() if isinstance(variance, torch.Tensor) else variance, dtype=np.float32)
      try:
        m, v = np.broadcast_arrays(m, v)
      except ValueError:
        raise ValueError(f"`mean` of shape {m.shape} and `variance` of shape {v.shape} do not broadcast") from None
      if axis is None and m.size != 1:
        raise ValueError(f"axis=None takes scalar statistics; got shape {m.shape}")
      if m.ndim > 1 and m.size != m.shape[-1]:
        raise ValueError(f"statistics of shape {m.shape} do not lie along the last axis")
      self._set_statistics(m.reshape(-1), v.reshape(-1))
      self._given_scalar = m.size == 1

  # ---- state -----------------------------------------------------------------------------------------------------
  def _allocate(self, f: int) -> None:
    dev = _device(self._device)
    self.mean = torch.zeros((f,), dtype=torch.float32, device=dev)
    self.variance = torch.ones((f,), dtype=torch.float32, device=dev)
    self._scale = torch.ones((f,), dtype=torch.float32, device=dev)
    self.count = torch.zeros((), dtype=torch.int64, device=dev)
    self.moments = torch.zeros((f, 3), dtype=torch.float64, device=dev)
    self._workspace = None

  def _set_statistics(self, m: np.ndarray, v: np.ndarray) -> None:
    """Given statistics: the scale is taken on the host, where the f32 square root is the correctly rounded one."""
    self._allocate(m.size)
    m, v = np.ascontiguousarray(m, np.float32), np.ascontiguousarray(v, np.float32)
    with np.errstate(invalid="ignore"):
      scale = np.maximum(np.sqrt(v), np.float32(EPSILON))
    self.mean.copy_(torch.from_numpy(m))
    self.variance.copy_(torch.from_numpy(v))
    self._scale.copy_(torch.from_numpy(scale.astype(np.float32)))
    self._ready = True

  def _features_of(self, x: torch.Tensor) -> int:
    if self.axis is None:
      return 1
    if x.ndim == 0:
      raise ValueError("axis=-1 needs input with at least one axis")
    return int(x.shape[-1])

  def reset_state(self) -> None:
    if self.moments is not None:
      _lib.check(_lib.load().tfrs_moments_reset(_lib.ptr(self.moments), self.moments.shape[0], _lib.current_stream()))
      self.mean.zero_()
      self.variance.fill_(1.0)
      self._scale.fill_(1.0)
      self.count.zero_()
    self._ready = self._given_scalar = False

  def update_state(self, batch) -> None:
    """Folds one batch into the running moments: two launches, no host read."""
    dev = self.moments.device if self.moments is not None else _device(self._device)
    x = _as_numeric(_values_of(batch), dev)
    f = self._features_of(x)
    if self.moments is None:
      if f < 1:
        raise ValueError("the last axis is empty")
      self._allocate(f)
    elif self.moments.shape[0] != f:
      raise ValueError(f"the layer keeps statistics of {self.moments.shape[0]} features; got a batch with {f}")
    lib = _lib.load()
    if self._workspace is None:      # sized for the largest batch there is: the size stops growing at the group cap
      nbytes = lib.tfrs_moments_workspace_bytes(1 << 62, f)
      self._workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=self.moments.device)
    _lib.check(lib.tfrs_moments_update(_lib.ptr(x), _DTYPE_CODES[x.dtype], x.numel() // f, f, _lib.ptr(self.moments),
                                       _lib.ptr(self._workspace), self._workspace.numel() * 8,
                                       _lib.current_stream()))

  def finalize_state(self) -> None:
    if self.moments is None:
      return
    _lib.check(_lib.load().tfrs_moments_finalize(_lib.ptr(self.moments), self.moments.shape[0], _lib.ptr(self.mean),
                                                 _lib.ptr(self.variance), _lib.ptr(self._scale),
                                                 _lib.current_stream()))
    self.count.copy_(self.moments[0, 0])
    self._ready = True

  def adapt(self, data) -> None:
    """Statistics of ``data``: a tensor, an array, or an iterable of batches (all with the same last axis)."""
    self.reset_state()
    for batch in _batches(data):
      self.update_state(batch)
    if self.moments is None:
      raise ValueError("`adapt` needs at least one batch")
    self.finalize_state()

  # ---- call ------------------------------------------------------------------------------------------------------
  def forward(self, inputs) -> torch.Tensor:
    if not self._ready or self.mean is None:
      raise RuntimeError("Normalization has no statistics yet: pass `mean` and `variance` or call `adapt(data)`")
    if not self.mean.is_cuda:
      raise RuntimeError("recommenders_amd ops need a GPU; there is no CPU fallback.")
    x = _as_numeric(inputs, self.mean.device)
    if not self._given_scalar and self._features_of(x) != self.mean.numel():
      raise ValueError(f"the layer keeps statistics of {self.mean.numel()} features; the input's last axis has "
                       f"{self._features_of(x)}")
    return _Normalize.apply(x, self.mean, self._scale, self.invert)

  # ---- persistence -------------------------------------------------------------------------------------------------
  def get_extra_state(self):
    return {"ready": self._ready, "given_scalar": self._given_scalar}

  def set_extra_state(self, state):
    self._ready, self._given_scalar = bool(state["ready"]), bool(state.get("given_scalar", False))

  def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
    loaded = state_dict.get(prefix + "mean")
    if loaded is not None:          # the feature count is part of the state: make room for it
      self._allocate(loaded.numel())
    super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
    if loaded is not None:          # the scale is derived, never stored: on the host, as for given statistics
      v = self.variance.detach().cpu().numpy()
      with np.errstate(invalid="ignore"):
        self._scale.copy_(torch.from_numpy(np.maximum(np.sqrt(v), np.float32(EPSILON)).astype(np.float32)))
