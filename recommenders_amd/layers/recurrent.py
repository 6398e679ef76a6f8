"""Recurrent layers on MI355X.

``GRU`` mirrors ``tf.keras.layers.GRU`` as the reference's sequential retrieval tutorial uses it
(``docs/examples/sequential_retrieval.ipynb``: ``Embedding -> GRU(embedding_dimension)`` over the last ten watched
movies): Keras' default arithmetic (``reset_after=True``, ``tanh`` / ``sigmoid``), gate order ``z, r, h``, weights
``kernel [E, 3U]``, ``recurrent_kernel [U, 3U]``, ``bias [2, 3U]`` in Keras' order and shapes, and Keras' mask rule
(a masked step carries the state and repeats the previous output).

``LSTM`` mirrors ``tf.keras.layers.LSTM`` the same way: gate order ``i, f, c, o``, ``kernel [E, 4U]``,
``recurrent_kernel [U, 4U]``, ``bias [4U]``, two states ``h`` and ``c``, both carried over a masked step.

A forward call is the input projection of ALL time steps as one GEMM (``dense``) plus ONE recurrence launch
(``tfrs_gru_fwd``, csrc/gru.hip; ``tfrs_lstm_fwd``, csrc/lstm.hip); a backward call is one recurrence launch
(``tfrs_gru_bwd`` / ``tfrs_lstm_bwd``) plus two ``dense_backward`` calls: the input side, and the recurrent weight
gradient ``H_prev^T @ dG`` over all time steps at once (the LSTM's ``dG`` is the input side's ``da`` itself).  No host
synchronisation and no allocation besides outputs and saved tensors, so the layers run inside a captured step.
"""

import math
from typing import Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.layers.feature_interaction.dcn import dense, dense_backward

MAX_UNITS = 64       # TFRS_GRU_MAX_UNITS and TFRS_LSTM_MAX_UNITS of include/tfrs_hip.h


def _orthogonal_blocks(units: int, gates: int = 3) -> torch.Tensor:
  """``[U, gates U]``: every gate's ``[U, U]`` block is an orthogonal matrix (QR of a normal draw, signs fixed by R's
  diagonal as Keras' ``Orthogonal`` does).  Drawn on the host: no solver library on the device path."""
  blocks = []
  for _ in range(gates):
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


class _LSTMFn(torch.autograd.Function):
  """``(x, kernel, recurrent_kernel, bias, h0, c0) -> (h, c)`` or ``(sequence, h, c)``."""

  @staticmethod
  def forward(ctx, x, kernel, rk, bias, h0, c0, mask, need_seq, backwards):
    ctx.set_materialize_grads(False)
    b, t, e = x.shape
    u = rk.shape[0]
    dev = x.device
    kernel, rk = kernel.contiguous(), rk.contiguous()
    x2 = x.contiguous().reshape(b * t, e)
    xp = dense(x2, kernel, bias) if b * t else torch.empty((0, 4 * u), dtype=torch.float32, device=dev)
    train = any(ctx.needs_input_grad[:6])
    h = torch.empty((b, u), dtype=torch.float32, device=dev)
    c = torch.empty((b, u), dtype=torch.float32, device=dev)
    seq = torch.empty((b, t, u), dtype=torch.float32, device=dev) if need_seq else None
    saved = torch.empty((6, b, t, u), dtype=torch.float32, device=dev) if train else None      # i, f, g, o, c_prev, h_prev
    h0 = h0.contiguous() if h0 is not None else None
    c0 = c0.contiguous() if c0 is not None else None
    sv = [saved[i] for i in range(6)] if train else [None] * 6
    _lib.check(_lib.load().tfrs_lstm_fwd(
        _lib.ptr(xp), _lib.ptr(rk), _lib.ptr(mask), _lib.ptr(h0), _lib.ptr(c0), b, t, u, 1 if backwards else 0,
        _lib.ptr(seq), _lib.ptr(h), _lib.ptr(c), *[_lib.ptr(s) for s in sv], _lib.current_stream()))
    if t == 0 and b:          # no step ran: the state is the initial one
      h = h0.clone() if h0 is not None else torch.zeros_like(h)
      c = c0.clone() if c0 is not None else torch.zeros_like(c)
    ctx.save_for_backward(x2, kernel, rk, mask, saved)
    ctx.shape, ctx.need_seq, ctx.backwards, ctx.has_bias = (b, t, e, u), need_seq, bool(backwards), bias is not None
    return (seq, h, c) if need_seq else (h, c)

  @staticmethod
  def backward(ctx, *grads):
    x2, kernel, rk, mask, saved = ctx.saved_tensors
    b, t, e, u = ctx.shape
    dev = x2.device
    dseq, dh, dc = [g.contiguous() if g is not None else None for g in (grads if ctx.need_seq else (None,) + grads)]
    da = torch.empty((b * t, 4 * u), dtype=torch.float32, device=dev)
    dh0 = torch.empty((b, u), dtype=torch.float32, device=dev)
    dc0 = torch.empty((b, u), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tfrs_lstm_bwd(
        _lib.ptr(rk), _lib.ptr(mask), *[_lib.ptr(saved[i]) for i in range(5)], _lib.ptr(dseq), _lib.ptr(dh),
        _lib.ptr(dc), b, t, u, 1 if ctx.backwards else 0, _lib.ptr(da), _lib.ptr(dh0), _lib.ptr(dc0),
        _lib.current_stream()))
    if t == 0 and b:
      dh0 = dh.clone() if dh is not None else torch.zeros_like(dh0)
      dc0 = dc.clone() if dc is not None else torch.zeros_like(dc0)
    need_x, need_k, need_rk, need_b, need_h0, need_c0 = ctx.needs_input_grad[:6]
    need_b = need_b and ctx.has_bias
    dx = dk = drk = dbias = None
    if need_x or need_k or need_b:
      dx, dk, dbias = dense_backward(x2, kernel, da, need_x, need_k, need_b)
      if dx is not None:
        dx = dx.reshape(b, t, e)
    if need_rk:
      # one bias, one pre-activation gradient: the recurrent weight gradient is H_prev^T @ da on the SAME buffer
      _, drk, _ = dense_backward(saved[5].reshape(b * t, u), rk, da, False, True, False)
    return dx, dk, drk, dbias, (dh0 if need_h0 else None), (dc0 if need_c0 else None), None, None, None


class _Recurrent(torch.nn.Module):
  """What ``GRU`` and ``LSTM`` share: the options, the list of what is not built, and the weight plumbing.  A subclass
  sets ``_gates`` and gives ``_bias_shape`` / ``_initial_bias``."""

  _gates = 0

  def __init__(self, units, return_sequences, return_state, go_backwards, use_bias, device, activation,
               recurrent_activation, dropout, recurrent_dropout, stateful, unroll, time_major):
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

  def _bias_shape(self):
    raise NotImplementedError

  def _initial_bias(self) -> torch.Tensor:
    return torch.zeros(self._bias_shape(), dtype=torch.float32)

  def build(self, in_dim: int, device=None, initialize: bool = True) -> None:
    """``kernel``: glorot_uniform, ``recurrent_kernel``: orthogonal, ``bias``: zeros.  ``initialize=False`` only
    allocates (the caller fills the parameters: ``set_weights``, ``load_state_dict``)."""
    dev = torch.device(device) if device is not None else (self._device or torch.device("cuda"))
    u, n = self.units, self._gates * self.units
    shapes = [(int(in_dim), n), (u, n)] + ([self._bias_shape()] if self.use_bias else [])
    if initialize:
      lim = math.sqrt(6.0 / (int(in_dim) + n))
      values = [torch.empty(shapes[0], dtype=torch.float32).uniform_(-lim, lim), _orthogonal_blocks(u, self._gates),
                self._initial_bias()]
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
    u, n = self.units, self._gates * self.units
    if weights[0].dim() != 2 or weights[0].shape[1] != n:
      raise ValueError(f"`kernel` must be [input_dim, {n}]; got {tuple(weights[0].shape)}")
    if tuple(weights[1].shape) != (u, n):
      raise ValueError(f"`recurrent_kernel` must be [{u}, {n}]; got {tuple(weights[1].shape)}")
    if self.use_bias and tuple(weights[2].shape) != self._bias_shape():
      raise ValueError(f"`bias` must be {list(self._bias_shape())}; got {tuple(weights[2].shape)}")
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

  def _inputs(self, x: torch.Tensor, mask: Optional[torch.Tensor]):
    """``x`` as float32 ``[batch, time, features]`` on the GPU (the layer built on first use) and ``mask`` as
    contiguous bool ``[batch, time]`` beside it."""
    name = type(self).__name__
    if x.dim() != 3:
      raise ValueError(f"{name} expects [batch, time, features]; got {tuple(x.shape)}")
    if not x.is_cuda:
      raise RuntimeError("recommenders_amd ops need tensors on the GPU; there is no CPU fallback.")
    b, t, e = x.shape
    if not self.built:
      self.build(e, self._device or x.device)
    if e != self.kernel.shape[0]:
      raise ValueError(f"{name} was built for {self.kernel.shape[0]} input features; got {e}")
    x = x.to(torch.float32)
    if mask is not None:
      if tuple(mask.shape) != (b, t):
        raise ValueError(f"`mask` must be [batch, time] = {(b, t)}; got {tuple(mask.shape)}")
      if mask.dtype != torch.bool:
        mask = mask != 0
      mask = mask.to(x.device).contiguous()
    return x, mask

  def _state(self, state: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    if tuple(state.shape) != (x.shape[0], self.units):
      raise ValueError(f"`initial_state` must be [batch, units] = {(x.shape[0], self.units)}; got "
                       f"{tuple(state.shape)}")
    return state.to(x.device, torch.float32)


class GRU(_Recurrent):
  """``tf.keras.layers.GRU(units, return_sequences=False, return_state=False, go_backwards=False,
  use_bias=True)`` with Keras' defaults for everything else; what is not built raises ``NotImplementedError`` at
  construction, with the argument named."""

  _gates = 3

  def __init__(self, units: int, return_sequences: bool = False, return_state: bool = False,
               go_backwards: bool = False, use_bias: bool = True, device: Optional[torch.device] = None,
               activation="tanh", recurrent_activation="sigmoid", dropout: float = 0.0,
               recurrent_dropout: float = 0.0, stateful: bool = False, unroll: bool = False,
               reset_after: bool = True, time_major: bool = False):
    if not reset_after:
      raise NotImplementedError("reset_after=False is not built; only Keras' default reset_after=True")
    super().__init__(units, return_sequences, return_state, go_backwards, use_bias, device, activation,
                     recurrent_activation, dropout, recurrent_dropout, stateful, unroll, time_major)

  def _bias_shape(self):
    return (2, 3 * self.units)

  def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None,
              initial_state: Optional[torch.Tensor] = None):
    x, mask = self._inputs(x, mask)
    if initial_state is not None:
      if isinstance(initial_state, (list, tuple)):
        (initial_state,) = initial_state
      initial_state = self._state(initial_state, x)
    out = _GRUFn.apply(x, self.kernel, self.recurrent_kernel, self.bias, initial_state, mask, self.return_sequences,
                       self.go_backwards)
    seq, last = out if self.return_sequences else (None, out)
    first = seq if self.return_sequences else last
    return (first, last) if self.return_state else first

  call = forward


class LSTM(_Recurrent):
  """``tf.keras.layers.LSTM(units, return_sequences=False, return_state=False, go_backwards=False, use_bias=True,
  unit_forget_bias=True)`` with Keras' defaults for everything else; what is not built raises
  ``NotImplementedError`` at construction, with the argument named.  ``initial_state`` is ``[h0, c0]``;
  ``return_state=True`` returns ``(output, h, c)``.  The sequence output repeats at a masked step and, as in Keras, is
  zero before a row's first unmasked step, whatever the initial state."""

  _gates = 4

  def __init__(self, units: int, return_sequences: bool = False, return_state: bool = False,
               go_backwards: bool = False, use_bias: bool = True, unit_forget_bias: bool = True,
               device: Optional[torch.device] = None, activation="tanh", recurrent_activation="sigmoid",
               dropout: float = 0.0, recurrent_dropout: float = 0.0, stateful: bool = False, unroll: bool = False,
               time_major: bool = False):
    super().__init__(units, return_sequences, return_state, go_backwards, use_bias, device, activation,
                     recurrent_activation, dropout, recurrent_dropout, stateful, unroll, time_major)
    self.unit_forget_bias = bool(unit_forget_bias)

  def _bias_shape(self):
    return (4 * self.units,)

  def _initial_bias(self) -> torch.Tensor:
    bias = super()._initial_bias()
    if self.unit_forget_bias:
      bias[self.units:2 * self.units] = 1.0
    return bias

  def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, initial_state=None):
    x, mask = self._inputs(x, mask)
    h0 = c0 = None
    if initial_state is not None:
      if not isinstance(initial_state, (list, tuple)) or len(initial_state) != 2:
        raise ValueError("`initial_state` must be [h0, c0]")
      h0, c0 = (self._state(s, x) for s in initial_state)
    out = _LSTMFn.apply(x, self.kernel, self.recurrent_kernel, self.bias, h0, c0, mask, self.return_sequences,
                        self.go_backwards)
    first, h, c = out if self.return_sequences else (out[0],) + tuple(out)
    return (first, h, c) if self.return_state else first

  call = forward
