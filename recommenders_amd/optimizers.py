"""Optimizers for the training step of ``tfrs.Model`` on MI355X.

``Adagrad`` restates ``tf.keras.optimizers.Adagrad`` as the reference's quickstart uses it
(``README.md:84``: ``tfrs.Model.compile(optimizer=tf.keras.optimizers.Adagrad(0.5))``, applied
in ``models/base.py:77-78``):

    accumulator starts at ``initial_accumulator_value`` (0.1); per step
    ``acc += g * g ;  var -= learning_rate * g / sqrt(acc + epsilon)``   (epsilon = 1e-7)

and, like TensorFlow's handling of ``IndexedSlices`` gradients of embedding lookups, only
touches the rows that were looked up: duplicate ids are summed first, then the update is
applied once per unique row.  For parameters of :class:`recommenders_amd.layers.embedding.Embedding`
the gradient never exists as a dense ``[vocab, dim]`` tensor -- the lookup's backward hands
``(ids, grad_rows)`` slices to the optimizer, which runs the fused sort + segmented
scatter-add + Adagrad kernel (``tfrs_embedding_scatter_add_unsorted_dlr`` with ``adagrad=1``; every sparse update of
this module is in ``csrc/sparse_update.hip``, the dense halves in ``csrc/table_update.hip``).
Dense parameters (Cross kernels, MLPs) take the same formula element-wise.

The reference's tests do not pin Adagrad numerics ("parity unpinned"); the
formula above is the one of ``tf.keras.optimizers.Adagrad`` since TF 2.11 and of tf-keras
(``variable.assign_sub(lr * grad / sqrt(accumulator + epsilon))``); the test oracle restates the same
formula.  TF <= 2.10 (the reference's release script pins TF 2.9.0, ``tools/build_scripts/release.sh:6``)
runs the optimizer_v2 kernel ``ResourceApplyAdagradV2``, which divides by ``sqrt(acc) + epsilon``:
``Adagrad(..., legacy=True)`` selects that form -- it is also ``torch.optim.Adagrad``'s, which
``tests/test_ops_gpu.py`` cross-checks it against as an independent implementation;
``tools/tf_reference_vectors.py`` writes the TensorFlow-side vectors of both forms for a maintainer with
TensorFlow installed (``tests/test_tf_vectors.py`` consumes them when present).

``SGD``, ``Adam`` and ``Ftrl`` are the other three table optimizers the reference's embedding layer names
(``layers/embedding/tpu_embedding_layer.py:37-49, 101-112``: ``'sgd'``, ``'adagrad'``, ``'adam'``, ``'ftrl'``).  They take
the same ``(ids, rows)`` slices through one set of HIP kernels that is templated on the rule (``csrc/table_rules.h``;
``tfrs_table_update_sparse`` on both routes of the Adagrad update, ``tfrs_table_update_dense_multi`` for dense
parameters).  All arithmetic is float32 in the written operation order, without contraction; duplicate ids are summed
first, in occurrence order from +0 -- the bits of the Adagrad path's sum, which on the sorted route cuts a run longer
than a piece of max(32, 2^k >= d) positions at fixed positions into occurrence-order pieces and adds those in order;
ids outside ``[0, vocab)`` are ignored.

    SGD    ``w -= lr * g``                                               (``tf.keras.optimizers.SGD.update_step``,
                                                                          momentum 0)
    Adam   ``alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)``          (``tf.keras.optimizers.Adam.update_step``;
           ``m += (g - m) * (1 - beta_1)``                                ``t = iterations + 1``)
           ``v += (g * g - v) * (1 - beta_2)``
           ``w -= m * alpha / (sqrt(v) + epsilon)``
    Ftrl   ``g' = g + 2 * shrink * w ;  n' = n + g * g``                 (``tf.keras.optimizers.Ftrl.update_step``,
           ``lin += g' - (n'^p - n^p) / lr * w``                          ``p = -learning_rate_power``,
           ``q = n'^p / lr + 2 * l2r``                                    ``l2r = l2 + beta / (2 lr)``)
           ``w = (clip(lin, -l1, l1) - lin) / q ;  n = n'``

On tables Adam is LAZY -- only looked-up rows have ``m``, ``v`` and ``w`` touched, a looked-up row whose summed gradient
is exactly zero included: ``tf.tpu.experimental.embedding.Adam(lazy_adam=True)``, the table optimizer the reference's
layer builds, and ``torch.optim.SparseAdam``; Keras's own Adam on ``IndexedSlices`` decays every row's moments.  ``t`` is
one counter per optimizer, advanced once per ``step()``; it lives ON THE DEVICE (a host counter would be frozen by graph
replay): the one-thread kernel ``tfrs_adam_tick`` increments it and writes ``alpha``, computed in float64 from the
integer ``t`` and rounded once, into a device float the update kernels read.  Ftrl is row-sparse on tables as
TensorFlow's ``ResourceSparseApplyFtrlV2`` is (untouched rows are not written; dense Keras Ftrl would re-solve them);
``learning_rate_power`` is ``-0.5`` or ``0`` (a general ``powf`` has no error bound this project can state).  These
numerics are reference-unpinned like Adagrad's: the reference's tests hold no vector for them, and the formulas are
Keras's and TensorFlow's own; ``tools/tf_reference_vectors.py`` writes vectors for a maintainer with TensorFlow.

``RowWiseAdagrad`` is Adagrad with ONE accumulator scalar per table row -- FBGEMM's and torchrec's "exact row-wise
Adagrad", what DLRM-style models on one GPU are usually trained with: the state of a ``[vocab, d]`` table is ``vocab``
floats instead of ``vocab * d`` (26 M x 128: 104 MB against 13.3 GB), and the sparse update moves the weights and the
gradient only.  It is not in the reference; its numerics are reference-unpinned and the formula is the contract.  With
``G`` the row's summed gradient (duplicates summed first, the bits of the other optimizers' sums) and ``d`` its width,
all in float32 in the written order without contraction:

    ``s = (sum_j G_j * G_j) / d ;  acc' = acc + s``                      (acc: float32 ``[vocab]``, starts at
    ``den = sqrt(acc' + epsilon)``   (``legacy``: ``sqrt(acc') + epsilon``)    ``initial_accumulator_value``)
    ``scale = lr / den ;  w_j' = w_j - scale * G_j``                     (one division per row)

The order of the ``d`` additions is fixed per route (``csrc/table_rules.h``).  Every parameter must be 2-D (a model's
other tensors go to another optimizer through ``experimental.optimizers.CompositeOptimizer``); the slices of a table go
through ``tfrs_rowwise_adagrad_sparse`` (the same sort and piece-wise sums as the other rules, then one lane group per
run; the row scan for small tables), a dense ``.grad`` through ``tfrs_rowwise_adagrad_dense``; ids outside
``[0, vocab)`` are ignored, untouched rows are not written, a row whose summed gradient is exactly zero keeps its bits.

Schedules.  ``learning_rate`` of every optimizer here (and of ``experimental.optimizers.ClippyAdagrad``) is one of: a
float; a ``schedules.LearningRateSchedule`` (``recommenders_amd/schedules.py``, also ``optimizers.schedules``); a 0-d
float32 device tensor; a zero-argument callable returning such a tensor, called once -- the two dynamic forms of the
reference (``layers/embedding/tpu_embedding_layer.py:287-328``).  A float is passed to the kernels by value, exactly as
before: no extra launch, no extra state.  Anything else lives on the device: the optimizer creates, in its
constructor, an int64 counter ``state[first parameter]["iterations"]`` (``Adam``: its ``step``) and two floats
``state[first parameter of the group]["learning_rate"]``; at the head of ``step()`` the one-thread kernel
``tfrs_lr_tick`` evaluates every such group's schedule at the counter in float64, rounds once to f32 into the group's
float (for ``Ftrl`` also ``2 * (l2 + beta / (2 lr))`` from that f32), and advances the counter once; the update kernels
read the float at entry (their device-lr instantiations; ``Adam``'s tick evaluates the schedule at ``t - 1`` and derives
``alpha`` from it in the same kernel).  A captured step therefore replays the whole schedule, and ``Model.fit`` re-captures
only when the schedule OBJECT is replaced.  CPU tensors evaluate the schedule on the host at a host counter
(``float(np.float32(schedule(t)))`` into the same formulas); a parameter on the GPU that is off the kernel route reads
the device float back (a synchronisation).  ``iterations`` is ``None`` for a float learning rate (except ``Adam``'s).
"""

import ctypes
from typing import Any, Dict, Iterable, Optional, Tuple
import weakref

import numpy as np
import torch

from recommenders_amd import schedules
from recommenders_amd.layers import embedding as emb


def _adagrad_dense_multi(items, lr: float, eps: float, mode: int, lr_dev: Optional[torch.Tensor] = None) -> None:
  from recommenders_amd import _lib
  n = len(items)
  vp, i64a = ctypes.c_void_p * n, ctypes.c_int64 * n
  args = (n, vp(*[p.data_ptr() for p, _, _ in items]), vp(*[a.data_ptr() for _, a, _ in items]),
          vp(*[g.data_ptr() for _, _, g in items]), i64a(*[p.numel() for p, _, _ in items]), float(lr))
  _lib.check(_lib.load().tfrs_adagrad_dense_multi_dlr(*args, _lib.ptr(lr_dev), float(eps), int(mode),
                                                      _lib.current_stream()))
  SliceOwningOptimizer._wrote(*[p for p, _, _ in items])


def _is_dynamic(lr) -> bool:
  """A learning rate the kernels read from the device: a schedule or a tensor (anything else is a float by value)."""
  return isinstance(lr, (schedules.LearningRateSchedule, torch.Tensor))


class SliceOwningOptimizer(torch.optim.Optimizer):
  """What every optimizer of this package that takes the ``(ids, rows)`` slices of embedding lookups shares
  (``Adagrad``, ``experimental.optimizers.ClippyAdagrad``): ownership of the tables' sparse-gradient mode
  (``_tfrs_sparse_grad`` / ``_tfrs_slices`` / ``_tfrs_sparse_owner``), ``close``, the per-parameter accumulator,
  ``reset_state_``, ``zero_grad`` and the version bumps after raw-pointer writes.  Subclasses pass their
  hyper-parameters as ``defaults`` (``initial_accumulator_value`` among them, for those that keep an accumulator), name
  the constructor arguments in ``_CONFIG`` and implement ``step``; the route test, the torch route's dedupe of slices and
  the re-cast of loaded state are here as well."""

  _COUNTER = "iterations"     # the state key of the device counter (``Adam``: its ``step``)
  _CONFIG = ()                # the constructor's keyword arguments, all of them keys of a parameter group
  # state that keeps its own dtype whatever the parameter's is (``load_state_dict``); subclasses add to it
  _STATE_DTYPES = {"iterations": torch.int64, "learning_rate": torch.float32, "step": torch.int64,
                   "alpha": torch.float32}

  def __init__(self, params: Iterable, defaults: dict):
    if defaults.get("initial_accumulator_value", 0.0) < 0.0:
      raise ValueError("initial_accumulator_value must be non-negative")
    if "learning_rate" in defaults:
      defaults["learning_rate"] = self._coerce_learning_rate(defaults["learning_rate"])
    super().__init__(params, defaults)
    for group in self.param_groups:
      for p in group["params"]:
        if getattr(p, "_tfrs_embedding", False):
          p._tfrs_sparse_grad = True        # the lookup's backward now emits slices
          p._tfrs_slices = []
          # the LATEST optimizer built on a table owns its sparse-gradient mode: an older one
          # that is closed / collected afterwards must not switch it off
          p._tfrs_sparse_owner = weakref.ref(self)

  # -- learning rates that are not a float (module docstring, "Schedules") ---------------------------------------------
  @staticmethod
  def _coerce_learning_rate(lr):
    """A float stays a float; a ``LearningRateSchedule`` or a 0-d float32 tensor is kept as it is; a zero-argument
    callable is called ONCE and must return such a tensor (the reference's second form: the kernels then read the
    tensor every step); a ``{"class_name", "config"}`` dict (``get_config``) is deserialized."""
    if isinstance(lr, dict):
      lr = schedules.deserialize(lr)
    if isinstance(lr, schedules.LearningRateSchedule):
      return lr
    if callable(lr) and not isinstance(lr, torch.Tensor):
      lr = lr()
      if not isinstance(lr, torch.Tensor):
        raise ValueError("learning_rate: a callable must return a 0-d float32 tensor (called once; the tensor is read "
                         "every step); for a Python function of the step use schedules.Tabulated.from_callable")
    if isinstance(lr, torch.Tensor):
      if lr.dim() != 0 or lr.dtype != torch.float32:
        raise ValueError(f"learning_rate: a tensor must be 0-d float32; got shape {tuple(lr.shape)} {lr.dtype}")
      return lr
    return float(lr)

  def _init_learning_rate(self) -> None:
    """End of every constructor: with a learning rate that is not a float, the counter and the groups' device floats are
    created NOW -- state that exists before a capture's warm-up is snapshotted and rolled back."""
    for group in self.param_groups:     # (a group given as a dict brings its own learning rate)
      group["learning_rate"] = self._coerce_learning_rate(group["learning_rate"])
    dynamic = [g for g in self.param_groups if _is_dynamic(g["learning_rate"])]
    if not dynamic:
      return
    params = [p for group in self.param_groups for p in group["params"]]
    if len({p.device for p in params}) > 1:
      self.close()
      raise ValueError(f"{type(self).__name__}: with a learning-rate schedule all parameters must live on one device "
                       "(the counter is one device tensor that the kernels read); build one optimizer per device")
    for group in dynamic:
      lr = group["learning_rate"]
      if isinstance(lr, torch.Tensor) and params and lr.device != params[0].device:
        self.close()
        raise ValueError(f"learning_rate: the tensor lives on {lr.device}, the parameters on {params[0].device}")
    self._counter()
    for group in dynamic:
      self._lr_buffer(group)

  def _counter(self) -> torch.Tensor:
    first = self.param_groups[0]["params"][0]
    state = self.state[first]
    if self._COUNTER not in state:
      state[self._COUNTER] = torch.zeros((), dtype=torch.int64, device=first.device)
    return state[self._COUNTER]

  def _lr_buffer(self, group) -> torch.Tensor:
    """The group's two device floats: [0] the learning rate of the step, [1] Ftrl's ``2 * l2r`` derived from it."""
    first = group["params"][0]
    state = self.state[first]
    if "learning_rate" not in state:
      state["learning_rate"] = torch.zeros((2,), dtype=torch.float32, device=first.device)
    return state["learning_rate"]

  @property
  def iterations(self) -> Optional[torch.Tensor]:
    """Steps taken so far, a 0-d int64 tensor on the parameters' device that the tick kernel advances (so a replayed
    step counts); ``None`` with a constant float learning rate, which keeps no counter (``Adam`` always has one)."""
    first = self.param_groups[0]["params"][0]
    return self.state[first].get(self._COUNTER) if first in self.state else None

  @staticmethod
  def _schedule_args(lr, device):
    """``(kind, params, table, table_len)`` of ``tfrs_lr_tick`` for a schedule or a learning-rate tensor."""
    if isinstance(lr, torch.Tensor):
      return schedules.KIND_EXTERNAL, (ctypes.c_double * 8)(), lr, 1
    kind, params, _ = lr._device_description()
    table = lr._device_table(device)
    return (kind, (ctypes.c_double * 8)(*(list(params) + [0.0] * (8 - len(params)))), table,
            0 if table is None else table.numel())

  def _ftrl_terms(self, group) -> Optional[Tuple[float, float]]:
    """``(l2, beta)`` when the tick also has to write ``2 * (l2 + beta / (2 lr))`` (``Ftrl``)."""
    return None

  def _tick(self) -> None:
    """Head of ``step()``: every group whose learning rate is not a float gets this step's value written into its
    buffer, all of them at the same ``iterations``, which then advances by one.  On the device by ``tfrs_lr_tick``; for
    CPU parameters on the host (``float32(schedule(t))`` in NumPy float64)."""
    dynamic = [g for g in self.param_groups if _is_dynamic(g["learning_rate"])]
    if not dynamic:
      return
    counter = self._counter()
    for i, group in enumerate(dynamic):
      lr, buf, last = group["learning_rate"], self._lr_buffer(group), i == len(dynamic) - 1
      ftrl = self._ftrl_terms(group)
      if counter.is_cuda:
        from recommenders_amd import _lib
        kind, params, table, table_len = self._schedule_args(lr, counter.device)
        _lib.check(_lib.load().tfrs_lr_tick(_lib.ptr(counter), _lib.ptr(buf), kind, params, _lib.ptr(table), table_len,
                                            0 if ftrl is None else 1, *(ftrl or (0.0, 0.0)), 1 if last else 0,
                                            _lib.current_stream()))
        torch.autograd.graph.increment_version(buf)
        torch.autograd.graph.increment_version(counter)
      else:
        value = np.float32(lr) if isinstance(lr, torch.Tensor) else np.float32(lr(int(counter)))
        buf[0] = float(value)
        if ftrl is not None:
          buf[1] = float(np.float32(2.0 * (ftrl[0] + ftrl[1] / (2.0 * float(value)))))
        if last:
          counter.add_(1)

  def _step_lr(self, group) -> Tuple[float, Optional[torch.Tensor]]:
    """``(lr, lr_dev)`` for the kernels of this step: a float learning rate and ``None``, or 0.0 and the group's device
    float (after ``_tick``)."""
    lr = group["learning_rate"]
    if not _is_dynamic(lr):
      return float(lr), None
    return 0.0, self._lr_buffer(group)

  def _host_group(self, group) -> dict:
    """The group with its learning rate as a host float, for the torch formulas (CPU tensors, parameters off the kernel
    route; reading a device float synchronises)."""
    if not _is_dynamic(group["learning_rate"]):
      return group
    return dict(group, learning_rate=float(self._lr_buffer(group)[0]))

  def _config_learning_rate(self, lr):
    if isinstance(lr, schedules.LearningRateSchedule):
      return schedules.serialize(lr)
    return float(lr)

  def get_config(self) -> Dict[str, Any]:
    group = self.param_groups[0] if self.param_groups else self.defaults
    config = {k: group[k] for k in self._CONFIG}
    config["learning_rate"] = self._config_learning_rate(config["learning_rate"])
    return config

  @classmethod
  def from_config(cls, params: Iterable, config: Dict[str, Any]):
    return cls(params, **config)

  def load_state_dict(self, state_dict) -> None:
    super().load_state_dict(state_dict)
    # (torch casts loaded state to the parameter's dtype: the entries of _STATE_DTYPES are taken from the saved state
    # itself, in their own dtype, onto the parameter's device)
    saved = state_dict["state"]
    ids = [i for group in state_dict["param_groups"] for i in group["params"]]
    params = [p for group in self.param_groups for p in group["params"]]
    for i, p in zip(ids, params):
      for key, value in saved.get(i, {}).items():
        if key in self._STATE_DTYPES:
          self.state[p][key] = value.detach().clone().to(device=p.device, dtype=self._STATE_DTYPES[key])

  @staticmethod
  def _closure_loss(closure):
    """Head of every ``step(closure)``."""
    if closure is None:
      return None
    with torch.enable_grad():
      return closure()

  @staticmethod
  def _on_kernel_route(p, state_tensors, g) -> bool:
    """Whether parameter ``p`` with its per-parameter state and the gradient (or gradient rows) ``g`` can go to the HIP
    kernels; anything else takes the torch formulas."""
    return (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse
            and p.is_contiguous() and all(s.is_contiguous() for s in state_tensors) and g.device == p.device)

  @staticmethod
  def _wrote(*tensors) -> None:
    """Version counters of tensors the kernels wrote through raw pointers, so that anything keyed on them (Streaming's
    packed-block cache over views of a table) sees the change."""
    for t in tensors:
      torch.autograd.graph.increment_version(t)

  @staticmethod
  def _summed_slices(p, ids, rows, dtype):
    """The torch route's view of the slices of table ``p``: ``(unique ids, their summed rows [u, d])`` -- ids outside
    ``[0, vocab)`` dropped, duplicates summed first in ``dtype`` (on the CPU ``index_add_`` adds in occurrence order)."""
    flat = ids.reshape(-1).long()
    g = rows.reshape(flat.numel(), p.shape[1])
    keep = (flat >= 0) & (flat < p.shape[0])
    flat, g = flat[keep], g[keep]
    uniq, inverse = torch.unique(flat, return_inverse=True)
    return uniq, torch.zeros((uniq.numel(), p.shape[1]), dtype=dtype, device=g.device).index_add_(0, inverse,
                                                                                                  g.to(dtype))

  def _owns(self, p) -> bool:
    owner = getattr(p, "_tfrs_sparse_owner", None)
    return owner is not None and owner() is self

  def close(self) -> None:
    """Hands the embedding tables back to dense gradients: after ``close()`` (also called when the
    optimizer is garbage-collected) a lookup's backward produces an ordinary ``.grad`` again, so
    the tables can be trained by another optimizer.  Only tables this optimizer still owns are
    released: a newer ``Adagrad`` built on the same parameters keeps its sparse mode and its
    pending slices."""
    for group in self.param_groups:
      for p in group["params"]:
        if getattr(p, "_tfrs_sparse_grad", False) and self._owns(p):
          p._tfrs_sparse_grad = False
          p._tfrs_slices = []
          p._tfrs_sparse_owner = None

  def __del__(self):
    try:
      self.close()
    except Exception:   # interpreter shutdown
      pass

  def _accumulator(self, p: torch.Tensor, init: float) -> torch.Tensor:
    state = self.state[p]
    if "accumulator" not in state:
      state["accumulator"] = torch.full_like(p, init)
    return state["accumulator"]

  @torch.no_grad()
  def reset_state_(self) -> None:
    """Accumulators back to ``initial_accumulator_value`` in place (same storage)."""
    for group in self.param_groups:
      for p in group["params"]:
        acc = self.state[p].get("accumulator") if p in self.state else None
        if acc is not None:
          acc.fill_(group["initial_accumulator_value"])
        if p in self.state and "iterations" in self.state[p]:
          self.state[p]["iterations"].zero_()

  def bump_table_versions(self) -> None:
    """Version counters of every table this optimizer updates through raw pointers.  ``step()`` does it
    for the tables it touched; a HIP-graph REPLAY of a captured step runs no host code, so
    ``Model.make_graphed_train_step`` calls this after every replay -- anything keyed on the counters
    (Streaming's packed-block cache over detached views of a trained table) then sees the change."""
    for group in self.param_groups:
      for p in group["params"]:
        if getattr(p, "_tfrs_sparse_grad", False):
          torch.autograd.graph.increment_version(p)

  def zero_grad(self, set_to_none: bool = True) -> None:
    super().zero_grad(set_to_none=set_to_none)
    for group in self.param_groups:
      for p in group["params"]:
        if getattr(p, "_tfrs_sparse_grad", False):
          p._tfrs_slices.clear()

  @staticmethod
  def _merged_slices(p):
    """The pending slices of table ``p`` as one ``(ids, rows)`` pair (``None`` when there are none); clears them."""
    slices = getattr(p, "_tfrs_slices", None)
    if not slices:
      return None
    if len(slices) == 1:
      ids, rows = slices[0]
    else:   # the same table looked up several times: one combined IndexedSlices
      ids = torch.cat([s[0].reshape(-1) for s in slices])
      rows = torch.cat([s[1].reshape(-1, p.shape[1]) for s in slices])
    slices.clear()
    return ids, rows


class Adagrad(SliceOwningOptimizer):
  """``tf.keras.optimizers.Adagrad(learning_rate, initial_accumulator_value, epsilon)``."""

  _CONFIG = ("learning_rate", "initial_accumulator_value", "epsilon", "legacy")

  def __init__(self, params: Iterable, learning_rate=0.001,
               initial_accumulator_value: float = 0.1, epsilon: float = 1e-7, legacy: bool = False):
    super().__init__(params, dict(learning_rate=learning_rate,
                                  initial_accumulator_value=float(initial_accumulator_value),
                                  epsilon=float(epsilon), legacy=bool(legacy)))
    self._init_learning_rate()

  @torch.no_grad()
  def step(self, closure=None):
    loss = self._closure_loss(closure)
    self._tick()
    for group in self.param_groups:
      (lr, lr_dev), eps, legacy = self._step_lr(group), group["epsilon"], group.get("legacy", False)
      sparse = []     # (table, accumulator, grad rows, ids) of every looked-up table of the group
      touched = []
      for p in group["params"]:
        acc = self._accumulator(p, group["initial_accumulator_value"])
        merged = self._merged_slices(p)
        if merged is not None:
          ids, rows = merged
          sparse.append((p.data, acc, rows, ids))
          touched.append(p)
      if sparse:
        emb.adagrad_sparse_update_multi_(sparse, lr, eps, legacy, lr_dev=lr_dev)   # small tables: one launch for all
        self._wrote(*touched)
      dense = []      # (parameter, accumulator, gradient) of every dense parameter of the group on a GPU
      for p in group["params"]:
        acc = self._accumulator(p, group["initial_accumulator_value"])
        if p.grad is not None:
          g = p.grad
          if self._on_kernel_route(p, [acc], g):
            dense.append((p, acc, g.contiguous()))
            continue
          acc.addcmul_(g, g)
          p.addcdiv_(g, torch.sqrt(acc) + eps if legacy else torch.sqrt(acc + eps),
                     value=-self._host_group(group)["learning_rate"])
      # every dense parameter of the group in one launch per 32 tensors (``tfrs_adagrad_dense_multi``): the four torch
      # kernels per tensor above were 72 launches of a DCN-v2 step
      for lo in range(0, len(dense), 32):
        _adagrad_dense_multi(dense[lo:lo + 32], lr, eps, 2 if legacy else 1, lr_dev)
    return loss


class RowWiseAdagrad(SliceOwningOptimizer):
  """Adagrad with ONE accumulator scalar per table row ("exact row-wise Adagrad"; module docstring).  Every parameter is
  2-D; ``state[p]["accumulator"]`` is float32 ``[p.shape[0]]``."""

  _CONFIG = Adagrad._CONFIG
  _STATE_DTYPES = dict(SliceOwningOptimizer._STATE_DTYPES, accumulator=torch.float32)    # (whatever the table is)

  def __init__(self, params: Iterable, learning_rate=0.001, initial_accumulator_value: float = 0.1,
               epsilon: float = 1e-7, legacy: bool = False):
    if epsilon < 0.0:
      raise ValueError("RowWiseAdagrad: epsilon must be non-negative")
    super().__init__(params, dict(learning_rate=learning_rate,
                                  initial_accumulator_value=float(initial_accumulator_value),
                                  epsilon=float(epsilon), legacy=bool(legacy)))
    for group in self.param_groups:
      for p in group["params"]:
        if p.dim() != 2:
          self.close()
          raise ValueError(f"RowWiseAdagrad keeps one accumulator per ROW of a 2-D parameter; got a parameter of shape "
                           f"{tuple(p.shape)}.  Give biases and other tensors to another optimizer (e.g. Adagrad) and "
                           "pair the two through experimental.optimizers.CompositeOptimizer")
    self._init_learning_rate()

  def _accumulator(self, p: torch.Tensor, init: float) -> torch.Tensor:
    state = self.state[p]
    if "accumulator" not in state:
      state["accumulator"] = torch.full((p.shape[0],), init, dtype=torch.float32, device=p.device)
    return state["accumulator"]

  @staticmethod
  def _formula(w, acc, g, lr: float, eps: float, legacy: bool):
    """The module docstring's rule on same-rowed ``w [r, d]``, ``acc [r]``, ``g [r, d]`` in torch ops, float32 in the
    kernels' operation order (the order of the ``d`` additions inside the sum is torch's): ``(new w, new acc)``."""
    g = g.to(torch.float32)
    s = (g * g).sum(dim=1) / torch.full_like(acc, float(g.shape[1]))     # (a tensor: a true division, not * (1 / d))
    acc = acc + s
    den = torch.sqrt(acc) + eps if legacy else torch.sqrt(acc + eps)
    scale = torch.full_like(acc, lr) / den
    return (w.to(torch.float32) - scale[:, None] * g).to(w.dtype), acc

  def _sparse_call(self, p, acc, ids, rows, lr, lr_dev, eps, legacy) -> None:
    from recommenders_amd import _lib
    lib = _lib.load()
    d = p.shape[1]
    flat, g = emb._flat_slices(ids, rows, d)
    n = flat.numel()
    rowscan = 1 if emb._use_rowscan(p.shape[0], n, d) else 0
    # (the row scan needs no workspace: a small table's step is host-bound, an allocation less is measurable)
    ws = None if rowscan else torch.empty((lib.tfrs_table_update_workspace_bytes(n, 0),), dtype=torch.uint8,
                                          device=p.device)
    _lib.check(lib.tfrs_rowwise_adagrad_sparse(
        _lib.ptr(g), _lib.ptr(flat), 1 if flat.dtype == torch.int64 else 0, n, d, p.shape[0], _lib.ptr(p.data),
        _lib.ptr(acc), float(lr), _lib.ptr(lr_dev), float(eps), 2 if legacy else 1, rowscan, _lib.ptr(ws),
        0 if ws is None else ws.numel(), _lib.current_stream()))
    self._wrote(p, acc)

  def _sparse_fallback(self, p, acc, ids, rows, lr, eps, legacy) -> None:
    uniq, summed = self._summed_slices(p, ids, rows, torch.float32)
    w, a = self._formula(p.data[uniq], acc[uniq], summed, lr, eps, legacy)
    p.data[uniq] = w
    acc[uniq] = a

  def _dense_call(self, p, acc, g, lr, lr_dev, eps, legacy) -> None:
    from recommenders_amd import _lib
    _lib.check(_lib.load().tfrs_rowwise_adagrad_dense(
        _lib.ptr(p.data), _lib.ptr(acc), _lib.ptr(g), p.shape[0], p.shape[1], float(lr), _lib.ptr(lr_dev), float(eps),
        2 if legacy else 1, _lib.current_stream()))
    self._wrote(p, acc)

  @torch.no_grad()
  def step(self, closure=None):
    loss = self._closure_loss(closure)
    self._tick()
    for group in self.param_groups:
      (lr, lr_dev), eps, legacy = self._step_lr(group), group["epsilon"], group.get("legacy", False)
      host_lr = lambda: self._host_group(group)["learning_rate"]     # (reading a device float synchronises)
      for p in group["params"]:
        acc = self._accumulator(p, group["initial_accumulator_value"])
        merged = self._merged_slices(p)
        if merged is not None:
          ids, rows = merged
          if self._on_kernel_route(p, [acc], rows) and ids.device == p.device:
            self._sparse_call(p, acc, ids, rows, lr, lr_dev, eps, legacy)
          else:
            self._sparse_fallback(p, acc, ids.to(p.device), rows.to(p.device), host_lr(), eps, legacy)
        if p.grad is None:
          continue
        g = p.grad
        if self._on_kernel_route(p, [acc], g):
          self._dense_call(p, acc, g.contiguous(), lr, lr_dev, eps, legacy)
          continue
        w, a = self._formula(p.data, acc, g.to_dense() if g.is_sparse else g, host_lr(), eps, legacy)
        p.data.copy_(w)
        acc.copy_(a)
    return loss


class _RuleOptimizer(SliceOwningOptimizer):
  """What ``SGD``, ``Adam`` and ``Ftrl`` share: float32 parameters on the GPU go through the rule-templated kernels
  (``tfrs_table_update_sparse`` for the slices of a table, ``tfrs_table_update_dense_multi`` for up to 32 dense tensors
  per launch); a CPU tensor, a non-float32 or a non-contiguous parameter takes ``_formula`` in torch ops.  Every device
  tensor a step mutates is a tensor inside ``self.state[p]``: the snapshot of a graph capture rolls the warm-up back."""

  _RULE = -1        # the `rule` argument of the C entries
  _SLOTS = ()       # state keys of the per-element slots, in kernel order

  # -- what a rule defines ---------------------------------------------------------------------------------------------
  def _slot_init(self, group, key: str) -> float:
    return 0.0

  def _hyper(self, group):
    """The ``hyper_h`` floats of the C entries (``csrc/table_rules.h``)."""
    raise NotImplementedError

  def _formula(self, w, slots, g, group, alpha):
    """The module docstring's formula in torch ops, same operation order: ``(new w, [new slots])``."""
    raise NotImplementedError

  def _begin_step(self) -> None:
    self._tick()

  def _alpha(self, group):
    """The device floats the kernels read: Adam's ``alpha``; for ``SGD`` / ``Ftrl`` the group's learning-rate buffer
    when the learning rate is not a float (``None``: the kernels take ``hyper_h``)."""
    return self._step_lr(group)[1]

  # -- state -----------------------------------------------------------------------------------------------------------
  def _slots_of(self, p, group):
    state = self.state[p]
    for key in self._SLOTS:
      if key not in state:
        state[key] = torch.full_like(p, self._slot_init(group, key), memory_format=torch.contiguous_format)
    return [state[key] for key in self._SLOTS]

  @torch.no_grad()
  def reset_state_(self) -> None:
    """Slots back to their initial value and Adam's counter to 0, in place (same storage)."""
    for group in self.param_groups:
      for p in group["params"]:
        state = self.state[p] if p in self.state else {}
        for key in self._SLOTS:
          if key in state:
            state[key].fill_(self._slot_init(group, key))
        for key in ("step", "alpha", "iterations"):
          if key in state:
            state[key].zero_()

  # -- the update ------------------------------------------------------------------------------------------------------
  def _sparse_call(self, p, slots, ids, rows, hyper, alpha) -> None:
    from recommenders_amd import _lib
    lib = _lib.load()
    d = p.shape[1]
    flat, g = emb._flat_slices(ids, rows, d)
    n = flat.numel()
    rowscan = 1 if emb._use_rowscan(p.shape[0], n, d) else 0
    ws = torch.empty((lib.tfrs_table_update_workspace_bytes(n, rowscan),), dtype=torch.uint8, device=p.device)
    s0, s1 = (list(slots) + [None, None])[:2]
    _lib.check(lib.tfrs_table_update_sparse(
        self._RULE, hyper, _lib.ptr(alpha), _lib.ptr(g), _lib.ptr(flat), 1 if flat.dtype == torch.int64 else 0, n, d,
        p.shape[0], _lib.ptr(p.data), _lib.ptr(s0), _lib.ptr(s1), rowscan, _lib.ptr(ws), ws.numel(),
        _lib.current_stream()))
    self._wrote(p, *slots)

  def _sparse_fallback(self, p, slots, ids, rows, group, alpha) -> None:
    uniq, summed = self._summed_slices(p, ids, rows, rows.dtype)     # (the gradient's own precision, like the kernels)
    w, new = self._formula(p.data[uniq], [s[uniq] for s in slots], summed.to(p.dtype), group, alpha)
    p.data[uniq] = w
    for s, value in zip(slots, new):
      s[uniq] = value

  def _dense_call(self, items, hyper, alpha) -> None:
    from recommenders_amd import _lib
    n = len(items)
    vp, i64a = ctypes.c_void_p * n, ctypes.c_int64 * n
    slot = lambda k: vp(*[s[k].data_ptr() for _, s, _ in items]) if len(self._SLOTS) > k else None
    _lib.check(_lib.load().tfrs_table_update_dense_multi(
        self._RULE, hyper, _lib.ptr(alpha), n, vp(*[p.data_ptr() for p, _, _ in items]), slot(0), slot(1),
        vp(*[g.data_ptr() for _, _, g in items]), i64a(*[p.numel() for p, _, _ in items]), _lib.current_stream()))
    for p, slots, _ in items:
      self._wrote(p, *slots)

  @torch.no_grad()
  def step(self, closure=None):
    loss = self._closure_loss(closure)
    self._begin_step()
    for group in self.param_groups:
      hyper = (ctypes.c_float * 8)(*self._hyper(group))
      alpha = self._alpha(group)
      dense = []      # (parameter, slots, gradient) of every dense parameter of the group on the kernel route
      for p in group["params"]:
        slots = self._slots_of(p, group)
        merged = self._merged_slices(p)
        if merged is not None:
          ids, rows = merged
          if self._on_kernel_route(p, slots, rows) and ids.device == p.device:
            self._sparse_call(p, slots, ids, rows, hyper, alpha)
          else:
            self._sparse_fallback(p, slots, ids.to(p.device), rows.to(p.device), self._host_group(group), alpha)
        if p.grad is None:
          continue
        g = p.grad
        if self._on_kernel_route(p, slots, g):
          dense.append((p, slots, g.contiguous()))
          continue
        w, new = self._formula(p.data, slots, (g.to_dense() if g.is_sparse else g).to(p.dtype),
                               self._host_group(group), alpha)
        p.data.copy_(w)
        for s, value in zip(slots, new):
          s.copy_(value)
      for lo in range(0, len(dense), 32):
        self._dense_call(dense[lo:lo + 32], hyper, alpha)
    return loss


class SGD(_RuleOptimizer):
  """``tf.keras.optimizers.SGD(learning_rate)`` without momentum: ``w -= lr * g``."""

  _RULE = 0
  _CONFIG = ("learning_rate",)

  def __init__(self, params: Iterable, learning_rate=0.01, momentum: float = 0.0, nesterov: bool = False):
    if momentum != 0.0 or nesterov:
      raise NotImplementedError("SGD: momentum and nesterov are not implemented")
    super().__init__(params, dict(learning_rate=learning_rate))
    self._init_learning_rate()

  def _hyper(self, group):
    return [self._step_lr(group)[0]]

  def _formula(self, w, slots, g, group, alpha):
    return w - group["learning_rate"] * g, []


class Adam(_RuleOptimizer):
  """``tf.keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon)``; lazy on tables (module docstring).  The step
  counter ``state[first parameter]["step"]`` (int64) and each group's ``alpha`` live on the device."""

  _RULE = 1
  _SLOTS = ("m", "v")
  _CONFIG = ("learning_rate", "beta_1", "beta_2", "epsilon")
  _COUNTER = "step"

  def __init__(self, params: Iterable, learning_rate=0.001, beta_1: float = 0.9, beta_2: float = 0.999,
               epsilon: float = 1e-7):
    if not 0.0 <= beta_1 < 1.0 or not 0.0 <= beta_2 < 1.0:
      raise ValueError("Adam: beta_1 and beta_2 must be in [0, 1)")
    if epsilon < 0.0:
      raise ValueError("Adam: epsilon must be non-negative")
    super().__init__(params, dict(learning_rate=learning_rate, beta_1=float(beta_1), beta_2=float(beta_2),
                                  epsilon=float(epsilon)))
    if len({p.device for group in self.param_groups for p in group["params"]}) > 1:
      self.close()
      raise ValueError("Adam: all parameters must live on one device (the step counter is one device tensor that the "
                       "kernels read); build one Adam per device")
    self._init_learning_rate()
    for group in self.param_groups:
      if _is_dynamic(group["learning_rate"]):
        self._alpha(group)

  @property
  def iterations(self) -> torch.Tensor:
    """The device counter ``t`` (steps taken so far; 0-d int64)."""
    return self._counter()

  def _alpha(self, group) -> torch.Tensor:
    first = group["params"][0]
    state = self.state[first]
    if "alpha" not in state:
      state["alpha"] = torch.zeros((), dtype=torch.float32, device=first.device)
    return state["alpha"]

  def _begin_step(self) -> None:
    step = self._counter()
    for i, group in enumerate(self.param_groups):
      alpha = self._alpha(group)
      lr, b1, b2 = group["learning_rate"], group["beta_1"], group["beta_2"]
      dynamic = _is_dynamic(lr)
      if step.is_cuda:
        from recommenders_amd import _lib
        if dynamic:     # the schedule at t - 1 and alpha from its f32, in the one tick kernel
          buf = self._lr_buffer(group)
          kind, params, table, table_len = self._schedule_args(lr, step.device)
          _lib.check(_lib.load().tfrs_adam_tick_scheduled(
              _lib.ptr(step), _lib.ptr(alpha), _lib.ptr(buf), kind, params, _lib.ptr(table), table_len, b1, b2,
              1 if i == 0 else 0, _lib.current_stream()))
          self._wrote(buf)
        else:
          _lib.check(_lib.load().tfrs_adam_tick(_lib.ptr(step), _lib.ptr(alpha), lr, b1, b2, 1 if i == 0 else 0,
                                                _lib.current_stream()))
        self._wrote(step, alpha)
      else:
        if i == 0:
          step.add_(1)
        t = int(step)
        if dynamic:
          lr = float(np.float32(lr) if isinstance(lr, torch.Tensor) else np.float32(lr(t - 1)))
          self._lr_buffer(group)[0] = lr
        alpha.fill_(lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t))

  def _hyper(self, group):
    return [1.0 - group["beta_1"], 1.0 - group["beta_2"], group["epsilon"]]

  def _formula(self, w, slots, g, group, alpha):
    m, v = slots
    m = m + (g - m) * (1.0 - group["beta_1"])
    v = v + (g * g - v) * (1.0 - group["beta_2"])
    return w - m * alpha.to(w.dtype) / (torch.sqrt(v) + group["epsilon"]), [m, v]


class Ftrl(_RuleOptimizer):
  """``tf.keras.optimizers.Ftrl``; row-sparse on tables; ``learning_rate_power`` is ``-0.5`` or ``0`` (module
  docstring)."""

  _RULE = 2
  _SLOTS = ("accumulator", "linear")
  _CONFIG = ("learning_rate", "learning_rate_power", "initial_accumulator_value", "l1_regularization_strength",
             "l2_regularization_strength", "l2_shrinkage_regularization_strength", "beta")

  def __init__(self, params: Iterable, learning_rate=0.001, learning_rate_power: float = -0.5,
               initial_accumulator_value: float = 0.1, l1_regularization_strength: float = 0.0,
               l2_regularization_strength: float = 0.0, l2_shrinkage_regularization_strength: float = 0.0,
               beta: float = 0.0):
    if initial_accumulator_value < 0.0:
      raise ValueError("`initial_accumulator_value` needs to be positive or zero. Received: "
                       f"initial_accumulator_value={initial_accumulator_value}.")
    if learning_rate_power > 0.0:
      raise ValueError(f"`learning_rate_power` needs to be negative or zero. Received: "
                       f"learning_rate_power={learning_rate_power}.")
    for name, value in (("l1_regularization_strength", l1_regularization_strength),
                        ("l2_regularization_strength", l2_regularization_strength),
                        ("l2_shrinkage_regularization_strength", l2_shrinkage_regularization_strength),
                        ("beta", beta)):
      if value < 0.0:
        raise ValueError(f"`{name}` needs to be positive or zero. Received: {name}={value}.")
    learning_rate = self._coerce_learning_rate(learning_rate)
    if isinstance(learning_rate, float) and learning_rate <= 0.0:
      raise ValueError("Ftrl: learning_rate must be positive (the update divides by it)")
    if isinstance(learning_rate, schedules.LearningRateSchedule) and learning_rate.min_value() <= 0.0:
      raise ValueError(f"Ftrl: the learning-rate schedule must stay positive (the update divides by it); its "
                       f"min_value() is {learning_rate.min_value()}")
    if learning_rate_power not in (-0.5, 0.0):
      raise NotImplementedError("Ftrl: learning_rate_power must be -0.5 or 0 (a general powf has no error bound this "
                                "project can state)")
    super().__init__(params, dict(
        learning_rate=learning_rate, learning_rate_power=float(learning_rate_power),
        initial_accumulator_value=float(initial_accumulator_value),
        l1_regularization_strength=float(l1_regularization_strength),
        l2_regularization_strength=float(l2_regularization_strength),
        l2_shrinkage_regularization_strength=float(l2_shrinkage_regularization_strength), beta=float(beta)))
    self._init_learning_rate()

  def _ftrl_terms(self, group):
    return group["l2_regularization_strength"], group["beta"]

  def _slot_init(self, group, key: str) -> float:
    return group["initial_accumulator_value"] if key == "accumulator" else 0.0

  def _hyper(self, group):
    lr = group["learning_rate"]
    if _is_dynamic(lr):     # the kernels read lr and 2 * l2r from the group's device floats (``_tick``)
      return [0.0, group["l1_regularization_strength"], 0.0, 2.0 * group["l2_shrinkage_regularization_strength"],
              group["learning_rate_power"]]
    l2r = group["l2_regularization_strength"] + group["beta"] / (2.0 * lr)
    return [lr, group["l1_regularization_strength"], 2.0 * l2r, 2.0 * group["l2_shrinkage_regularization_strength"],
            group["learning_rate_power"]]

  def _formula(self, w, slots, g, group, alpha):
    n, lin = slots
    lr, l1, two_l2r, two_shrink, power = self._hyper(group)
    gp = g + two_shrink * w
    n2 = n + g * g
    pn2, pn = (torch.sqrt(n2), torch.sqrt(n)) if power != 0.0 else (torch.ones_like(n2), torch.ones_like(n))
    lin = lin + (gp - (pn2 - pn) / lr * w)
    q = pn2 / lr + two_l2r
    return (torch.clamp(lin, -l1, l1) - lin) / q, [n2, lin]
