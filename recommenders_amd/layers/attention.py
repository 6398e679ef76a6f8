"""Attention layers on MI355X.

``MultiHeadAttention`` mirrors ``tf.keras.layers.MultiHeadAttention`` as a sequence tower uses it (SASRec-style
self-attention over a history: ``Embedding(mask_zero=True) -> MultiHeadAttention(H, key_dim)(x, x,
use_causal_mask=True) -> last step``): Keras' weight shapes and order, ``scale = 1 / sqrt(key_dim)``, masks where
1 / True means "attend".  It is not the max-sim "multi-head" query of ``tasks.Retrieval`` / ``BruteForce`` (queries
``[B, H, D]``).

A forward call is the three projections through ``dense`` (the kernels ``[D, H, d]`` viewed as ``[D, H d]``), ONE
``tfrs_attention_fwd`` launch (csrc/attention.hip) on the projections' outputs as they are -- the kernel
reads a head's strided slice of ``[B T, H d]`` -- and one ``dense`` for the output projection.  A backward call is one
``tfrs_attention_bwd`` launch plus ``dense_backward`` calls.  No ``[B, H, Tq, Tk]`` score tensor exists in memory, in
either direction.  No host synchronisation and no allocation besides outputs and saved tensors, so the layer trains
inside a captured step.

One deviation from Keras: a query row that may attend to NO key comes out as zeros before the output
projection (Keras adds -1e9 to the scores, so the row becomes the mean of all value rows) and takes no gradient.
"""

import math
from typing import Optional

import torch

from recommenders_amd import _lib
from recommenders_amd.layers.feature_interaction.dcn import dense, dense_backward

MAX_SEQ = 128          # TFRS_ATTENTION_MAX_SEQ of include/tfrs_hip.h
MAX_HEAD_DIM = 64      # TFRS_ATTENTION_MAX_HEAD_DIM


def _initialize(spec, shape, fan_in: int, fan_out: int) -> torch.Tensor:
  t = torch.empty(shape, dtype=torch.float32)
  if callable(spec):
    return spec(t)
  if spec == "zeros":
    return t.zero_()
  if spec == "ones":
    return t.fill_(1.0)
  if spec == "glorot_uniform":
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return t.uniform_(-lim, lim)
  raise ValueError(f"Unknown initializer: {spec!r}")


class _AttentionFn(torch.autograd.Function):
  """``(query, value, key, 8 weights) -> output``; ``key`` and any bias may be ``None``."""

  @staticmethod
  def forward(ctx, query, value, key, wq, bq, wk, bk, wv, bv, wo, bo, attn_mask, q_mask, k_mask, causal):
    ctx.set_materialize_grads(False)
    b, tq, _ = query.shape
    tk = value.shape[1]
    heads, dk, dv, dout = wq.shape[1], wq.shape[2], wv.shape[2], wo.shape[2]
    dev = query.device
    flat = lambda t: None if t is None else t.contiguous().reshape(-1)
    w2 = [wq.contiguous().reshape(-1, heads * dk), wk.contiguous().reshape(-1, heads * dk),
          wv.contiguous().reshape(-1, heads * dv), wo.contiguous().reshape(heads * dv, dout)]
    ctx.shapes = (b, tq, tk, heads, dk, dv, dout)
    ctx.has_key = key is not None
    ctx.has_bias = bq is not None
    ctx.causal = bool(causal)
    if b == 0 or tq == 0:          # nothing to attend from: zeros plus the output bias, zero gradients
      ctx.in_shapes = (query.shape, value.shape, None if key is None else key.shape)
      y = torch.zeros((b, tq, dout), dtype=torch.float32, device=dev)
      return y + bo if bo is not None else y
    xq = query.contiguous().reshape(b * tq, -1)
    xv = value.contiguous().reshape(b * tk, -1)
    xk = xv if key is None else key.contiguous().reshape(b * tk, -1)
    q, k, v = dense(xq, w2[0], flat(bq)), dense(xk, w2[1], flat(bk)), dense(xv, w2[2], flat(bv))
    out = torch.empty((b * tq, heads * dv), dtype=torch.float32, device=dev)
    lse = torch.empty((b, heads, tq), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tfrs_attention_fwd(
        _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(attn_mask), _lib.ptr(q_mask), _lib.ptr(k_mask), b, tq, tk,
        heads, dk, dv, 1.0 / math.sqrt(dk), 1 if causal else 0, _lib.ptr(out), _lib.ptr(lse), _lib.current_stream()))
    y = dense(out, w2[3], bo).reshape(b, tq, dout)
    ctx.save_for_backward(xq, xk, xv, *w2, q, k, v, out, lse, attn_mask, q_mask, k_mask)
    return y

  @staticmethod
  def backward(ctx, dy):
    b, tq, tk, heads, dk, dv, dout = ctx.shapes
    need = ctx.needs_input_grad
    if dy is None:
      return (None,) * 15
    if b == 0 or tq == 0:
      zeros = lambda i, shape: torch.zeros(shape, dtype=torch.float32, device=dy.device) if need[i] and shape else None
      sq, sv, sk = ctx.in_shapes
      return (zeros(0, sq), zeros(1, sv), zeros(2, sk),
              zeros(3, (sq[2], heads, dk)), zeros(4, ctx.has_bias and (heads, dk)),
              zeros(5, ((sk or sv)[2], heads, dk)), zeros(6, ctx.has_bias and (heads, dk)),
              zeros(7, (sv[2], heads, dv)), zeros(8, ctx.has_bias and (heads, dv)),
              zeros(9, (heads, dv, dout)), zeros(10, ctx.has_bias and (dout,)), None, None, None, None)
    xq, xk, xv, wq, wk, wv, wo, q, k, v, out, lse, attn_mask, q_mask, k_mask = ctx.saved_tensors
    nb = lambda i: need[i] and ctx.has_bias
    dattn, dwo, dbo = dense_backward(out, wo, dy.contiguous().reshape(b * tq, dout), True, need[9], nb(10))
    dq, dkey, dval = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _lib.check(_lib.load().tfrs_attention_bwd(
        _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(attn_mask), _lib.ptr(q_mask), _lib.ptr(k_mask), _lib.ptr(out),
        _lib.ptr(lse), _lib.ptr(dattn), b, tq, tk, heads, dk, dv, 1.0 / math.sqrt(dk), 1 if ctx.causal else 0,
        _lib.ptr(dq), _lib.ptr(dkey), _lib.ptr(dval), _lib.current_stream()))

    def project_back(x, w, dyp, t, i_x, i_w, head_dim):
      if not (i_x is not None and need[i_x]) and not need[i_w] and not nb(i_w + 1):
        return None, None, None
      dx, dw, db = dense_backward(x, w, dyp, i_x is not None and need[i_x], need[i_w], nb(i_w + 1))
      return (None if dx is None else dx.reshape(b, t, -1), None if dw is None else dw.reshape(-1, heads, head_dim),
              None if db is None else db.reshape(heads, head_dim))

    dquery, dwq, dbq = project_back(xq, wq, dq, tq, 0, 3, dk)
    dvalue, dwv, dbv = project_back(xv, wv, dval, tk, 1, 7, dv)
    # without a `key` input the key projection reads `value`: its input gradient joins dvalue
    dkin, dwk, dbk = project_back(xk, wk, dkey, tk, 2 if ctx.has_key else (1 if need[1] else None), 5, dk)
    if not ctx.has_key and dkin is not None:
      dvalue, dkin = dvalue + dkin, None
    return (dquery, dvalue, dkin, dwq, dbq, dwk, dbk, dwv, dbv,
            None if dwo is None else dwo.reshape(heads, dv, dout), dbo, None, None, None, None)


class MultiHeadAttention(torch.nn.Module):
  """``tf.keras.layers.MultiHeadAttention(num_heads, key_dim, value_dim=None, use_bias=True, output_shape=None)``
  called as ``layer(query, value, key=None, attention_mask=None, use_causal_mask=False)``, plus the three per-step
  masks Keras takes from ``_keras_mask``: ``query_mask [B, Tq]``, ``value_mask`` and ``key_mask [B, Tk]``.  Sequences
  up to 128 steps and head dims up to 64; what is not built raises ``NotImplementedError`` with the argument named."""

  def __init__(self, num_heads: int, key_dim: int, value_dim: Optional[int] = None, use_bias: bool = True,
               output_shape=None, kernel_initializer="glorot_uniform", bias_initializer="zeros", dropout: float = 0.0,
               attention_axes=None, device: Optional[torch.device] = None, **kwargs):
    super().__init__()
    kwargs.pop("name", None)               # Keras call sites pass these; a torch module has no use for them
    if kwargs.pop("trainable", True) is not True or kwargs.pop("dtype", "float32") not in ("float32", torch.float32):
      raise NotImplementedError("only trainable=True and dtype='float32' are built")
    if kwargs:
      raise TypeError(f"MultiHeadAttention got unexpected keyword arguments {sorted(kwargs)}")
    if int(num_heads) < 1 or int(key_dim) < 1 or (value_dim is not None and int(value_dim) < 1):
      raise ValueError(f"`num_heads`, `key_dim` and `value_dim` must be positive; got {num_heads}, {key_dim}, "
                       f"{value_dim}")
    if dropout:
      raise NotImplementedError("dropout is not built")
    if attention_axes is not None:
      raise NotImplementedError("attention_axes is not built: attention runs over the one time axis of [B, T, D]")
    if isinstance(output_shape, (list, tuple)):
      if len(output_shape) != 1:
        raise NotImplementedError(f"output_shape={output_shape!r}: only one output axis is built")
      (output_shape,) = output_shape
    self.num_heads, self.key_dim = int(num_heads), int(key_dim)
    self.value_dim = int(value_dim) if value_dim is not None else int(key_dim)
    for name, d in (("key_dim", self.key_dim), ("value_dim", self.value_dim)):
      if d > MAX_HEAD_DIM:
        raise NotImplementedError(f"{name}={d}: the attention kernels hold head dims up to {MAX_HEAD_DIM} on chip")
    self.use_bias = bool(use_bias)
    self.output_dim = None if output_shape is None else int(output_shape)
    self.kernel_initializer, self.bias_initializer = kernel_initializer, bias_initializer
    self._device = device
    for name in self._names():
      self.register_parameter(name, None)

  def _names(self):
    kernels = ("query_kernel", "key_kernel", "value_kernel", "output_kernel")
    biases = ("query_bias", "key_bias", "value_bias", "output_bias")
    return [n for pair in zip(kernels, biases) for n in (pair if self.use_bias else pair[:1])]

  @property
  def built(self) -> bool:
    return self.query_kernel is not None

  def _shapes(self, query_dim: int, value_dim: int, key_dim: int):
    h, dk, dv = self.num_heads, self.key_dim, self.value_dim
    dout = self.output_dim if self.output_dim is not None else int(query_dim)
    shapes = {"query_kernel": (int(query_dim), h, dk), "query_bias": (h, dk), "key_kernel": (int(key_dim), h, dk),
              "key_bias": (h, dk), "value_kernel": (int(value_dim), h, dv), "value_bias": (h, dv),
              "output_kernel": (h, dv, dout), "output_bias": (dout,)}
    return [shapes[n] for n in self._names()]

  def build(self, query_dim: int, value_dim: Optional[int] = None, key_dim: Optional[int] = None, device=None,
            initialize: bool = True) -> None:
    """Kernels: ``kernel_initializer`` with Keras' fans (the axes before the last two are the receptive field);
    biases: ``bias_initializer``.  ``initialize=False`` only allocates (``set_weights``, ``load_state_dict``)."""
    dev = torch.device(device) if device is not None else (self._device or torch.device("cuda"))
    value_dim = query_dim if value_dim is None else value_dim
    key_dim = value_dim if key_dim is None else key_dim
    for name, shape in zip(self._names(), self._shapes(query_dim, value_dim, key_dim)):
      if not initialize:
        t = torch.empty(shape, dtype=torch.float32)
      elif name.endswith("bias"):
        t = _initialize(self.bias_initializer, shape, shape[0], shape[0])
      else:
        t = _initialize(self.kernel_initializer, shape, shape[0] * shape[1], shape[0] * shape[2])
      setattr(self, name, torch.nn.Parameter(t.to(dev)))

  def get_weights(self):
    """Keras' order: query kernel, bias, key kernel, bias, value kernel, bias, output kernel, bias (no biases with
    ``use_bias=False``), as numpy arrays."""
    if not self.built:
      return []
    return [getattr(self, n).detach().cpu().numpy().copy() for n in self._names()]

  def set_weights(self, weights) -> None:
    weights = [torch.as_tensor(w, dtype=torch.float32) for w in weights]
    names = self._names()
    if len(weights) != len(names):
      raise ValueError(f"expected {len(names)} weight arrays {names}; got {len(weights)}")
    kernels = dict(zip(names, weights))
    if any(kernels[n].dim() != 3 for n in ("query_kernel", "key_kernel", "value_kernel", "output_kernel")):
      raise ValueError("the four kernels must have three axes: [D, heads, d] and [heads, value_dim, Dout]")
    dims = [kernels[n].shape[0] for n in ("query_kernel", "value_kernel", "key_kernel")]
    if self.output_dim is None and kernels["output_kernel"].shape[2] != dims[0] and not self.built:
      self.output_dim = int(kernels["output_kernel"].shape[2])
    if not self.built:
      self.build(*dims, device=self._device or (torch.device("cuda") if torch.cuda.is_available()
                                                else torch.device("cpu")), initialize=False)
    for n, w in zip(names, weights):
      if tuple(w.shape) != tuple(getattr(self, n).shape):
        raise ValueError(f"`{n}` must be {tuple(getattr(self, n).shape)}; got {tuple(w.shape)}")
    with torch.no_grad():
      for n, w in zip(names, weights):
        getattr(self, n).copy_(w)

  def get_config(self):
    return {"num_heads": self.num_heads, "key_dim": self.key_dim, "value_dim": self.value_dim,
            "use_bias": self.use_bias, "output_shape": self.output_dim, "dropout": 0.0,
            "kernel_initializer": self.kernel_initializer, "bias_initializer": self.bias_initializer}

  @classmethod
  def from_config(cls, config):
    return cls(**config)

  def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
    ks = [state_dict.get(prefix + n) for n in ("query_kernel", "value_kernel", "key_kernel", "output_kernel")]
    if not self.built and all(k is not None for k in ks):          # lazily built: widths from the stored kernels
      if self.output_dim is None and ks[3].shape[2] != ks[0].shape[0]:
        self.output_dim = int(ks[3].shape[2])
      self.build(ks[0].shape[0], ks[1].shape[0], ks[2].shape[0], self._device or ks[0].device, initialize=False)
    super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

  @staticmethod
  def _mask(mask, shape, name, device):
    """``mask`` (bool or any integer dtype, non-zero = attend) as contiguous uint8 of ``shape`` on ``device``."""
    if mask is None:
      return None
    if not isinstance(mask, torch.Tensor):
      mask = torch.as_tensor(mask)
    if mask.dim() == len(shape) - 1:
      mask = mask[None]
    if mask.dim() != len(shape) or any(m not in (1, s) for m, s in zip(mask.shape, shape)):
      raise ValueError(f"`{name}` must be (broadcastable to) {tuple(shape)}; got {tuple(mask.shape)}")
    if mask.dtype != torch.bool:
      mask = mask != 0
    return mask.to(device).expand(shape).contiguous().view(torch.uint8)

  def forward(self, query: torch.Tensor, value: torch.Tensor, key: Optional[torch.Tensor] = None,
              attention_mask=None, query_mask=None, value_mask=None, key_mask=None, use_causal_mask: bool = False,
              return_attention_scores: bool = False, training=None):
    if return_attention_scores:
      raise NotImplementedError("return_attention_scores=True is not built: the scores never leave the kernel")
    for name, t in (("query", query), ("value", value), ("key", key)):
      if t is None:
        continue
      if t.dim() != 3:
        raise ValueError(f"MultiHeadAttention expects [batch, time, features]; `{name}` is {tuple(t.shape)}")
      if not t.is_cuda:
        raise RuntimeError("recommenders_amd ops need tensors on the GPU; there is no CPU fallback.")
    b, tq, tk = query.shape[0], query.shape[1], value.shape[1]
    if value.shape[0] != b or (key is not None and tuple(key.shape[:2]) != (b, tk)):
      raise ValueError(f"`query` {tuple(query.shape)}, `value` {tuple(value.shape)} and `key` "
                       f"{None if key is None else tuple(key.shape)} disagree in batch or key steps")
    for name, t in (("query steps", tq), ("key steps", tk)):
      if t > MAX_SEQ:
        raise NotImplementedError(f"{name} = {t}: the attention kernels hold sequences up to {MAX_SEQ} on chip")
    if tk == 0 and b and tq:
      raise ValueError("`value` has no steps to attend to")
    if not self.built:
      self.build(query.shape[2], value.shape[2], None if key is None else key.shape[2], self._device or query.device)
    dims = (self.query_kernel.shape[0], self.value_kernel.shape[0], self.key_kernel.shape[0])
    got = (query.shape[2], value.shape[2], (value if key is None else key).shape[2])
    if got != dims:
      raise ValueError(f"MultiHeadAttention was built for (query, value, key) features {dims}; got {got}")
    dev = query.device
    attn = self._mask(attention_mask, (b, tq, tk), "attention_mask", dev)
    qm = self._mask(query_mask, (b, tq), "query_mask", dev)
    km, vm = self._mask(key_mask, (b, tk), "key_mask", dev), self._mask(value_mask, (b, tk), "value_mask", dev)
    km = vm if km is None else (km if vm is None else km & vm)
    f32 = lambda t: None if t is None else t.to(torch.float32)
    return _AttentionFn.apply(f32(query), f32(value), f32(key), self.query_kernel, getattr(self, "query_bias", None),
                              self.key_kernel, getattr(self, "key_bias", None), self.value_kernel,
                              getattr(self, "value_bias", None), self.output_kernel,
                              getattr(self, "output_bias", None), attn, qm, km, bool(use_causal_mask))

  call = forward
