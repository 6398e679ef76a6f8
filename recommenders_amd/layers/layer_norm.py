"""Layer normalisation on MI355X.

``LayerNormalization`` mirrors ``tf.keras.layers.LayerNormalization`` over the last axis: per row of ``[..., D]``,
``(x - mean) / sqrt(var + epsilon) * gamma + beta`` with the two-pass moments of ``tf.nn.moments``.  It is what a
SASRec / BERT4Rec block puts around ``MultiHeadAttention`` and the feed-forward ``Dense`` pair, and it is not the
feature-wise preprocessing layer ``Normalization``.

One extension of Keras' call, for the residual stream of such a block: ``layer(x, residual=r)`` returns ``LN(x + r)``
and ``layer(x, residual=r, return_sum=True)`` returns ``(LN(x + r), x + r)`` -- the add happens in the registers of the
normalising kernel, so the sum costs one write and no read.

A forward call is ONE ``tfrs_layer_norm_fwd`` launch (csrc/layer_norm.hip); a backward call is
``tfrs_layer_norm_bwd`` (two launches, one without parameter gradients) and nothing else: ``dx`` is written once and
handed to ``x`` and ``residual`` alike.  The backward's workspace is allocated in the forward of a training call and
saved, so there is no host synchronisation and no allocation at replay: the layer trains inside a captured step.
"""

from typing import Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.layers.attention import _initialize

MAX_DIM = 8192          # TFRS_LAYER_NORM_MAX_DIM of include/tfrs_hip.h


class _LayerNormFn(torch.autograd.Function):
  """``(x, residual, gamma, beta) -> (y, sum)``; ``residual``, ``gamma`` and ``beta`` may be ``None``; ``sum`` is
  ``None`` unless ``return_sum``."""

  @staticmethod
  def forward(ctx, x, residual, gamma, beta, eps, return_sum):
    ctx.set_materialize_grads(False)
    d = x.shape[-1]
    n = x.numel() // d if d else 0
    x2 = x.contiguous().reshape(n, d)
    r2 = None if residual is None else residual.contiguous().reshape(n, d)
    gamma, beta = (None if t is None else t.contiguous() for t in (gamma, beta))
    need = ctx.needs_input_grad
    train = any(need[:4])
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    y = new(n, d)
    # the backward reads what was normalised: x itself, or the sum of a fused call
    s = new(n, d) if r2 is not None and (return_sum or train) else None
    mean, rstd = (new(n), new(n)) if train else (None, None)
    lib = _lib.load()
    _lib.check(lib.tfrs_layer_norm_fwd(_lib.ptr(x2), _lib.ptr(r2), _lib.ptr(gamma), _lib.ptr(beta), n, d, eps,
                                       _lib.ptr(y), _lib.ptr(s), _lib.ptr(mean), _lib.ptr(rstd),
                                       _lib.current_stream()))
    ctx.shape, ctx.fused = x.shape, r2 is not None
    if train:
      ws = None
      if need[2] or need[3]:
        ws = torch.empty(max(1, lib.tfrs_layer_norm_workspace_bytes(n, d) // 4), dtype=torch.float32, device=x.device)
      ctx.save_for_backward(x2 if s is None else s, mean, rstd, gamma, ws)
    if not return_sum:
      return y.reshape(x.shape), None
    return y.reshape(x.shape), s.reshape(x.shape)

  @staticmethod
  def backward(ctx, dy, dsum):
    need = ctx.needs_input_grad
    if dy is None and dsum is None:
      return (None,) * 6
    x, mean, rstd, gamma, ws = ctx.saved_tensors
    n, d = x.shape
    if dy is None:                          # only the sum output was used: its gradient passes straight through
      dx = dsum if need[0] or need[1] else None
      zeros = lambda i: torch.zeros(d, dtype=torch.float32, device=x.device) if need[i] else None
      return (dx if need[0] else None, dx if need[1] and ctx.fused else None, zeros(2), zeros(3), None, None)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    zero = n == 0                           # nothing launched: the caller zeroes the parameter gradients
    dx = new(n, d) if need[0] or need[1] else None
    dgamma = (torch.zeros(d, device=x.device) if zero else new(d)) if need[2] else None
    dbeta = (torch.zeros(d, device=x.device) if zero else new(d)) if need[3] else None
    dy2 = dy.contiguous().reshape(n, d)
    ds2 = None if dsum is None or dx is None else dsum.contiguous().reshape(n, d)
    _lib.check(_lib.load().tfrs_layer_norm_bwd(
        _lib.ptr(x), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(dy2), _lib.ptr(ds2), n, d,
        _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), 0 if ws is None else 4 * ws.numel(),
        _lib.current_stream()))
    dx = None if dx is None else dx.reshape(ctx.shape)
    return (dx if need[0] else None, dx if need[1] and ctx.fused else None, dgamma, dbeta, None, None)


class LayerNormalization(torch.nn.Module):
  """``tf.keras.layers.LayerNormalization(axis=-1, epsilon=1e-3, center=True, scale=True)`` over the last axis of an
  input of any rank >= 1, up to 8192 wide; called as ``layer(x)`` or, fused with the residual add,
  ``layer(x, residual=r, return_sum=False)``.  What is not built raises ``NotImplementedError`` with the argument
  named."""

  def __init__(self, axis=-1, epsilon: float = 1e-3, center: bool = True, scale: bool = True,
               beta_initializer="zeros", gamma_initializer="ones", device: Optional[torch.device] = None, **kwargs):
    super().__init__()
    kwargs.pop("name", None)               # Keras call sites pass these; a torch module has no use for them
    if kwargs.pop("trainable", True) is not True or kwargs.pop("dtype", "float32") not in ("float32", torch.float32):
      raise NotImplementedError("only trainable=True and dtype='float32' are built")
    if kwargs.pop("rms_scaling", False):
      raise NotImplementedError("rms_scaling is not built")
    if kwargs:
      raise TypeError(f"LayerNormalization got unexpected keyword arguments {sorted(kwargs)}")
    if isinstance(axis, (list, tuple)):
      if len(axis) != 1:
        raise NotImplementedError(f"axis={axis!r}: only the last axis is built")
      (axis,) = axis
    self.axis, self.epsilon = int(axis), float(epsilon)
    self.center, self.scale = bool(center), bool(scale)
    self.beta_initializer, self.gamma_initializer = beta_initializer, gamma_initializer
    self._device = device
    for name in self._names():
      self.register_parameter(name, None)
    self._dim = None

  def _names(self):
    return [n for n, on in (("gamma", self.scale), ("beta", self.center)) if on]

  @property
  def built(self) -> bool:
    return self._dim is not None

  def build(self, dim: int, device=None, initialize: bool = True) -> None:
    """``gamma`` and ``beta`` of ``[dim]``; ``initialize=False`` only allocates (``set_weights``,
    ``load_state_dict``)."""
    if int(dim) > MAX_DIM:
      raise NotImplementedError(f"a normalised axis of {int(dim)}: the layer-norm kernels hold rows up to {MAX_DIM}")
    dev = torch.device(device) if device is not None else (self._device or torch.device("cuda"))
    for name in self._names():
      spec = self.gamma_initializer if name == "gamma" else self.beta_initializer
      t = _initialize(spec, (int(dim),), int(dim), int(dim)) if initialize else torch.empty(int(dim))
      setattr(self, name, torch.nn.Parameter(t.to(dev)))
    self._dim = int(dim)

  def get_weights(self):
    """Keras' order ``[gamma, beta]`` (the one ``scale=False`` / ``center=False`` removes is absent), as numpy."""
    if not self.built:
      return []
    return [getattr(self, n).detach().cpu().numpy().copy() for n in self._names()]

  def set_weights(self, weights) -> None:
    weights = [torch.as_tensor(w, dtype=torch.float32) for w in weights]
    names = self._names()
    if len(weights) != len(names):
      raise ValueError(f"expected {len(names)} weight arrays {names}; got {len(weights)}")
    if any(w.dim() != 1 or w.shape != weights[0].shape for w in weights):
      raise ValueError(f"{names} must be vectors of one length; got {[tuple(w.shape) for w in weights]}")
    if not self.built and weights:
      self.build(weights[0].shape[0], device=self._device or (torch.device("cuda") if torch.cuda.is_available()
                                                              else torch.device("cpu")), initialize=False)
    with torch.no_grad():
      for n, w in zip(names, weights):
        if tuple(w.shape) != (self._dim,):
          raise ValueError(f"`{n}` must be ({self._dim},); got {tuple(w.shape)}")
        getattr(self, n).copy_(w)

  def get_config(self):
    return {"axis": self.axis, "epsilon": self.epsilon, "center": self.center, "scale": self.scale,
            "beta_initializer": self.beta_initializer, "gamma_initializer": self.gamma_initializer}

  @classmethod
  def from_config(cls, config):
    return cls(**config)

  def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
    stored = [state_dict.get(prefix + n) for n in self._names()]
    if not self.built and stored and all(t is not None for t in stored):     # lazily built: width from the vectors
      self.build(stored[0].shape[0], self._device or stored[0].device, initialize=False)
    super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

  def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, return_sum: bool = False,
              training=None):
    if x.dim() < 1:
      raise ValueError("LayerNormalization expects an input of rank >= 1")
    if self.axis not in (-1, x.dim() - 1):
      raise NotImplementedError(f"axis={self.axis} on an input of rank {x.dim()}: only the last axis is built")
    if return_sum and residual is None:
      raise ValueError("return_sum=True needs a `residual`")
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
      raise ValueError(f"`residual` {tuple(residual.shape)} must have the shape of `x` {tuple(x.shape)}")
    if not x.is_cuda or (residual is not None and not residual.is_cuda):
      raise RuntimeError("recommenders_amd ops need tensors on the GPU; there is no CPU fallback.")
    d = x.shape[-1]
    if d > MAX_DIM:
      raise NotImplementedError(f"a normalised axis of {d}: the layer-norm kernels hold rows up to {MAX_DIM}")
    if d < 1:
      raise ValueError("the normalised axis is empty")
    if not self.built:
      self.build(d, self._device or x.device)
    if d != self._dim:
      raise ValueError(f"LayerNormalization was built for a last axis of {self._dim}; got {d}")
    f32 = lambda t: None if t is None else t.to(torch.float32)
    y, s = _LayerNormFn.apply(f32(x), f32(residual), getattr(self, "gamma", None), getattr(self, "beta", None),
                              self.epsilon, bool(return_sum))
    return (y, s) if return_sum else y

  call = forward
