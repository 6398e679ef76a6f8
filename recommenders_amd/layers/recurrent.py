"""Recurrent layers on MI355X.

``GRU`` mirrors ``tf.keras.layers.GRU`` as the reference's sequential retrieval tutorial uses it
(``docs/examples/sequential_retrieval.ipynb``: ``Embedding -> GRU(embedding_dimension)`` over the last ten watched
movies): Keras' default arithmetic (``reset_after=True``, ``tanh`` / ``sigmoid``), gate order ``z, r, h``, weights
``kernel [E, 3U]``, ``recurrent_kernel [U, 3U]``, ``bias [2, 3U]`` in Keras' order and shapes, and Keras' mask rule
(a masked step carries the state and repeats the previous output).

A forward call is the input projection of ALL time steps as one GEMM (``dense``) plus ONE recurrence launch
(``tfrs_gru_fwd``, csrc/gru.hip); a backward call is one recurrence launch (``tfrs_gru_bwd``) plus two
``dense_backward`` calls: the input side, and the recurrent weight gradient ``H_prev^T @ dG`` over all time steps at
once.  No host synchronisation and no allocation besides outputs and saved tensors, so the layer runs inside a
captured step.
"""

import math
from typing import Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.layers.feature_interaction.dcn import dense, dense_backward

MAX_UNITS = 64       # TFRS_GRU_MAX_UNITS of include/tfrs_hip.h


def _orthogonal_blocks(units: int) -> torch.Tensor:
  """``[U, 3U]``: every gate's ``[U, U]`` block is an orthogonal matrix (QR of a normal draw, signs fixed by R's
  diagonal as Keras' ``Orthogonal`` does).  Drawn on the host: no solver library on the device path."""
  blocks = []
  for _ in range(3):
    q, r = torch.linalg.qr(torch.randn((units, units), dtype=torch.float64))
    blocks.append(q * torch.sign(torch.diagonal(r)).masked_fill(torch.diagonal(r) == 0, 1.0))
  return torch.cat(blocks, dim=1).to(torch.float32)


class _GRUFn(torch.autograd.Function):
  """``(x, kernel, recurrent_kernel, bias, h0) -> last`` or ``(sequence, last)``."""

  @staticmethod
  def forward(ctx, x, kernel, rk, bias, h0, mask, need_seq, backwards):
    ctx.set_materialize_grads(False)
    b, t, e = x.shape
    u = rk.shape[0]
    dev = x.device
    kernel, rk = kernel.contiguous(), rk.contiguous()
    x2 = x.contiguous().reshape(b * t, e)
    b0 = bias[0] if bias is not None else None
    b1 = bias[1] if bias is not None else None
    xp = dense(x2, kernel, b0) if b * t else torch.empty((0, 3 * u), dtype=torch.float32, device=dev)
    train = any(ctx.needs_input_grad[:5])
    last = torch.empty((b, u), dtype=torch.float32, device=dev)
    seq = torch.empty((b, t, u), dtype=torch.float32, device=dev) if need_seq else None
    saved = torch.empty((5, b, t, u), dtype=torch.float32, device=dev) if train else None
    if h0 is not None:
      h0 = h0.contiguous()
    sv = [saved[i] for i in range(5)] if train else [None] * 5
    _lib.check(_lib.load().tfrs_gru_fwd(
        _lib.ptr(xp), _lib.ptr(rk), _lib.ptr(b1), _lib.ptr(mask), _lib.ptr(h0), b, t, u, 1 if backwards else 0,
        _lib.ptr(seq), _lib.ptr(last), *[_lib.ptr(s) for s in sv], _lib.current_stream()))
    if t == 0 and b:          # no step ran: the state is the initial one
      last = h0.clone() if h0 is not None else torch.zeros_like(last)
    ctx.save_for_backward(x2, kernel, rk, mask, saved)
    ctx.shape, ctx.need_seq, ctx.backwards, ctx.has_bias = (b, t, e, u), need_seq, bool(backwards), bias is not None
    return (seq, last) if need_seq else last

  @staticmethod
  def backward(ctx, *grads):
    x2, kernel, rk, mask, saved = ctx.saved_tensors
    b, t, e, u = ctx.shape
    dev = x2.device
    dseq, dlast = grads if ctx.need_seq else (None, grads[0])
    dseq = dseq.contiguous() if dseq is not None else None
    dlast = dlast.contiguous() if dlast is not None else None
    da = torch.empty((b * t, 3 * u), dtype=torch.float32, device=dev)
    dg = torch.empty((b * t, 3 * u), dtype=torch.float32, device=dev)
    dh0 = torch.empty((b, u), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tfrs_gru_bwd(
        _lib.ptr(rk), _lib.ptr(mask), *[_lib.ptr(saved[i]) for i in range(5)], _lib.ptr(dseq), _lib.ptr(dlast),
        b, t, u, 1 if ctx.backwards else 0, _lib.ptr(da), _lib.ptr(dg), _lib.ptr(dh0), _lib.current_stream()))
    if t == 0 and b:
      dh0 = dlast.clone() if dlast is not None else torch.zeros_like(dh0)
    need_x, need_k, need_rk, need_b, need_h0 = ctx.needs_input_grad[:5]
    need_b = need_b and ctx.has_bias
    dx = dk = drk = dbias = None
    if need_x or need_k or need_b:
      dx, dk, db0 = dense_backward(x2, kernel, da, need_x, need_k, need_b)
      if dx is not None:
        dx = dx.reshape(b, t, e)
    if need_rk or need_b:
      # the recurrent weight gradient of ALL time steps as one product: H_prev^T @ dG, and dbias[1] its column sums
      _, drk, db1 = dense_backward(saved[4].reshape(b * t, u), rk, dg, False, need_rk, need_b)
    if need_b:
      dbias = torch.stack([db0, db1])
    return dx, dk, drk, dbias, (dh0 if need_h0 else None), None, None, None


class GRU(torch.nn.Module):
  """``tf.keras.layers.GRU(units, return_sequences=False, return_state=False, go_backwards=False,
  use_bias=True)`` with Keras' defaults for everything else; what is not built raises ``NotImplementedError`` at
  construction, with the argument named."""

  def __init__(self, units: int, return_sequences: bool = False, return_state: bool = False,
               go_backwards: bool = False, use_bias: bool = True, device: Optional[torch.device] = None,
               activation="tanh", recurrent_activation="sigmoid", dropout: float = 0.0,
               recurrent_dropout: float = 0.0, stateful: bool = False, unroll: bool = False,
               reset_after: bool = True, time_major: bool = False):
    super().__init__()
    if int(units) < 1:
      raise ValueError(f"`units` must be positive; got {units}")
    if activation != "tanh":
      raise NotImplementedError(f"activation={activation!r}: only 'tanh' is in the recurrence kernel")
    if recurrent_activation != "sigmoid":
      raise NotImplementedError(f"recurrent_activation={recurrent_activation!r}: only 'sigmoid' is in the "
                                "recurrence kernel")
    if dropout:
      raise NotImplementedError("dropout is not built")
    if recurrent_dropout:
      raise NotImplementedError("recurrent_dropout is not built")
    if stateful:
      raise NotImplementedError("stateful=True is not built; pass `initial_state`")
    if unroll:
      raise NotImplementedError("unroll=True is not built (the kernel walks the time steps itself)")
    if not reset_after:
      raise NotImplementedError("reset_after=False is not built; only Keras' default reset_after=True")
    if time_major:
      raise NotImplementedError("time_major=True is not built; inputs are [batch, time, features]")
    if int(units) > MAX_UNITS:
      raise NotImplementedError(f"units={units}: the recurrence kernels hold at most {MAX_UNITS} units on chip")
    self.units = int(units)
    self.return_sequences = bool(return_sequences)
    self.return_state = bool(return_state)
    self.go_backwards = bool(go_backwards)
    self.use_bias = bool(use_bias)
    self._device = device
    self.kernel: Optional[torch.nn.Parameter] = None
    self.recurrent_kernel: Optional[torch.nn.Parameter] = None
    self.bias: Optional[torch.nn.Parameter] = None

  @property
  def built(self) -> bool:
    return self.kernel is not None

  def build(self, in_dim: int, device=None, initialize: bool = True) -> None:
    """``kernel``: glorot_uniform, ``recurrent_kernel``: orthogonal, ``bias``: zeros.  ``initialize=False`` only
    allocates (the caller fills the parameters: ``set_weights``, ``load_state_dict``)."""
    dev = torch.device(device) if device is not None else (self._device or torch.device("cuda"))
    u = self.units
    shapes = [(int(in_dim), 3 * u), (u, 3 * u)] + ([(2, 3 * u)] if self.use_bias else [])
    if initialize:
      lim = math.sqrt(6.0 / (int(in_dim) + 3 * u))
      values = [torch.empty(shapes[0], dtype=torch.float32).uniform_(-lim, lim), _orthogonal_blocks(u),
                torch.zeros((2, 3 * u), dtype=torch.float32)]
      params = [v.to(dev) for v, _ in zip(values, shapes)]
    else:
      params = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
    self.kernel, self.recurrent_kernel = torch.nn.Parameter(params[0]), torch.nn.Parameter(params[1])
    if self.use_bias:
      self.bias = torch.nn.Parameter(params[2])

  def get_weights(self):
    """``[kernel, recurrent_kernel, bias]`` (no bias with ``use_bias=False``) as numpy arrays: Keras' order."""
    if not self.built:
      return []
    ws = [self.kernel, self.recurrent_kernel] + ([self.bias] if self.use_bias else [])
    return [w.detach().cpu().numpy().copy() for w in ws]

  def set_weights(self, weights) -> None:
    weights = [torch.as_tensor(w, dtype=torch.float32) for w in weights]
    want = 3 if self.use_bias else 2
    if len(weights) != want:
      raise ValueError(f"expected {want} weight arrays [kernel, recurrent_kernel{', bias' if self.use_bias else ''}]; "
                       f"got {len(weights)}")
    u = self.units
    if weights[0].dim() != 2 or weights[0].shape[1] != 3 * u:
      raise ValueError(f"`kernel` must be [input_dim, {3 * u}]; got {tuple(weights[0].shape)}")
    if tuple(weights[1].shape) != (u, 3 * u):
      raise ValueError(f"`recurrent_kernel` must be [{u}, {3 * u}]; got {tuple(weights[1].shape)}")
    if self.use_bias and tuple(weights[2].shape) != (2, 3 * u):
      raise ValueError(f"`bias` must be [2, {3 * u}]; got {tuple(weights[2].shape)}")
    if not self.built:
      self.build(weights[0].shape[0], self._device or (torch.device("cuda") if torch.cuda.is_available()
                                                       else torch.device("cpu")), initialize=False)
    if tuple(weights[0].shape) != tuple(self.kernel.shape):
      raise ValueError(f"`kernel` must be {tuple(self.kernel.shape)}; got {tuple(weights[0].shape)}")
    with torch.no_grad():
      for p, w in zip([self.kernel, self.recurrent_kernel] + ([self.bias] if self.use_bias else []), weights):
        p.copy_(w)

  def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
    k = state_dict.get(prefix + "kernel")
    if not self.built and k is not None:          # lazily built: take the input width from the stored kernel
      self.build(k.shape[0], self._device or k.device, initialize=False)
    super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

  def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None,
              initial_state: Optional[torch.Tensor] = None):
    if x.dim() != 3:
      raise ValueError(f"GRU expects [batch, time, features]; got {tuple(x.shape)}")
    if not x.is_cuda:
      raise RuntimeError("recommenders_amd ops need tensors on the GPU; there is no CPU fallback.")
    b, t, e = x.shape
    if not self.built:
      self.build(e, self._device or x.device)
    if e != self.kernel.shape[0]:
      raise ValueError(f"GRU was built for {self.kernel.shape[0]} input features; got {e}")
    x = x.to(torch.float32)
    if mask is not None:
      if tuple(mask.shape) != (b, t):
        raise ValueError(f"`mask` must be [batch, time] = {(b, t)}; got {tuple(mask.shape)}")
      if mask.dtype != torch.bool:
        mask = mask != 0
      mask = mask.to(x.device).contiguous()
    if initial_state is not None:
      if isinstance(initial_state, (list, tuple)):
        (initial_state,) = initial_state
      if tuple(initial_state.shape) != (b, self.units):
        raise ValueError(f"`initial_state` must be [batch, units] = {(b, self.units)}; got "
                         f"{tuple(initial_state.shape)}")
      initial_state = initial_state.to(x.device, torch.float32)
    out = _GRUFn.apply(x, self.kernel, self.recurrent_kernel, self.bias, initial_state, mask, self.return_sequences,
                       self.go_backwards)
    seq, last = out if self.return_sequences else (None, out)
    first = seq if self.return_sequences else last
    return (first, last) if self.return_state else first

  call = forward
