"""Learning-rate schedules that a captured train step replays (also ``recommenders_amd.optimizers.schedules``).

The reference supports a dynamic learning rate "for all optimizers" (``layers/embedding/tpu_embedding_layer.py:287-328``:
a ``tf.keras.optimizers.schedules`` object, or a zero-argument callable returning a scalar tensor;
``experimental/optimizers/clippy_adagrad.py:96-113`` types its argument ``Union[float, LearningRateSchedule]``).  Here
``Model.fit`` replays captured steps, and a learning rate passed to a kernel by value is frozen into the capture; so a
schedule is evaluated ON THE DEVICE: every optimizer of this package holds a device int64 ``iterations`` counter and one
device float per parameter group, the one-thread kernel ``tfrs_lr_tick`` at the head of ``step()`` writes the float from
the counter (in float64, rounded once to f32), and the update kernels read it.

The classes are Keras's (``tf.keras.optimizers.schedules``); TensorFlow is not installed where this package is tested,
so the formulas in the class docstrings are the contract (reference-unpinned, like the optimizers' own numerics).
``step`` is the optimizer's ``iterations`` before the update: 0 for the first ``step()``.  ``schedule(step)`` evaluates
on the host in NumPy float64 and returns a Python float; the device evaluates the same expression in the same order.
``Tabulated`` is the escape hatch for any other Python schedule: its values, rounded to f32 once, live in a device array.
"""

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# the `kind` argument of tfrs_lr_tick (csrc/table_update.hip)
KIND_EXTERNAL, KIND_EXPONENTIAL, KIND_INVERSE_TIME, KIND_POLYNOMIAL, KIND_COSINE, KIND_PIECEWISE, KIND_TABULATED = range(7)

_F = np.float64
# a PiecewiseConstantDecay of more than 7 boundaries is expanded into a table of boundaries[-1] + 2 values
_MAX_EXPANDED_TABLE = 1 << 22
# what ``min_value()`` answers for a positive schedule that decays TOWARDS 0 and is positive at every step (exponential,
# inverse time): the smallest positive double -- a valid lower bound in exact arithmetic that still tells "never zero"
# (``Ftrl`` divides by the learning rate and refuses a schedule whose bound is <= 0) from "reaches zero"
_APPROACHING_ZERO = float(np.nextafter(0.0, 1.0))


class LearningRateSchedule:
  """Base class: ``__call__(step) -> float`` on the host, ``get_config`` / ``from_config``, ``min_value()`` (an
  analytic lower bound over all steps >= 0) and the description the device kernels take."""

  def __call__(self, step: int) -> float:
    raise NotImplementedError

  def get_config(self) -> Dict[str, Any]:
    raise NotImplementedError

  @classmethod
  def from_config(cls, config: Dict[str, Any]) -> "LearningRateSchedule":
    return cls(**config)

  def min_value(self) -> float:
    raise NotImplementedError

  def _device_description(self) -> Tuple[int, List[float], Optional[np.ndarray]]:
    """``(kind, at most 8 doubles, float32 table or None)`` for ``tfrs_lr_tick``."""
    raise NotImplementedError

  def _device_table(self, device):
    """The description's table as a device tensor (built once per device; ``None`` without a table)."""
    import torch
    table = self._device_description()[2]
    if table is None:
      return None
    cache = self.__dict__.setdefault("_tables", {})
    key = str(device)
    if key not in cache:
      cache[key] = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(device)
    return cache[key]

  def __getstate__(self):     # (the device tables are a cache, not part of the schedule)
    return {k: v for k, v in self.__dict__.items() if k != "_tables"}


def _check_decay_steps(name: str, decay_steps) -> None:
  if not decay_steps > 0:
    raise ValueError(f"{name}: `decay_steps` must be > 0. Received: decay_steps={decay_steps}.")


class ExponentialDecay(LearningRateSchedule):
  """``p = step / decay_steps`` (floored when ``staircase``); ``lr = initial_learning_rate * decay_rate ** p``."""

  def __init__(self, initial_learning_rate: float, decay_steps: int, decay_rate: float, staircase: bool = False):
    _check_decay_steps(type(self).__name__, decay_steps)
    if not decay_rate > 0:
      raise ValueError(f"{type(self).__name__}: `decay_rate` must be > 0. Received: decay_rate={decay_rate}.")
    self.initial_learning_rate = float(initial_learning_rate)
    self.decay_steps = decay_steps
    self.decay_rate = float(decay_rate)
    self.staircase = bool(staircase)

  def _p(self, step):
    p = _F(step) / _F(self.decay_steps)
    return np.floor(p) if self.staircase else p

  def __call__(self, step: int) -> float:
    return float(_F(self.initial_learning_rate) * np.power(_F(self.decay_rate), self._p(step)))

  def get_config(self):
    return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                decay_rate=self.decay_rate, staircase=self.staircase)

  def min_value(self) -> float:
    # monotone in step: the value at step 0, or a bound of 0 that is approached and never reached (_approaching_zero)
    if self.initial_learning_rate <= 0.0:
      return self.initial_learning_rate if self.decay_rate <= 1.0 else -float("inf")
    return _APPROACHING_ZERO if self.decay_rate < 1.0 else self.initial_learning_rate

  _KIND = KIND_EXPONENTIAL

  def _device_description(self):
    return (self._KIND, [self.initial_learning_rate, float(self.decay_steps), self.decay_rate,
                         1.0 if self.staircase else 0.0], None)


class InverseTimeDecay(ExponentialDecay):
  """``p`` as for ``ExponentialDecay``; ``lr = initial_learning_rate / (1 + decay_rate * p)``."""

  _KIND = KIND_INVERSE_TIME

  def __call__(self, step: int) -> float:
    return float(_F(self.initial_learning_rate) / (_F(1.0) + _F(self.decay_rate) * self._p(step)))

  def min_value(self) -> float:
    if self.initial_learning_rate <= 0.0:
      return self.initial_learning_rate
    return _APPROACHING_ZERO     # decreasing towards 0, positive at every step


class PolynomialDecay(LearningRateSchedule):
  """Without ``cycle``: ``s = min(step, decay_steps)``, ``ds = decay_steps``; with ``cycle``: ``s = step``,
  ``ds = decay_steps * (1 if step == 0 else ceil(step / decay_steps))``;
  ``lr = (initial_learning_rate - end_learning_rate) * (1 - s / ds) ** power + end_learning_rate``."""

  def __init__(self, initial_learning_rate: float, decay_steps: int, end_learning_rate: float = 1e-4,
               power: float = 1.0, cycle: bool = False):
    _check_decay_steps("PolynomialDecay", decay_steps)
    if not power > 0:
      raise ValueError(f"PolynomialDecay: `power` must be > 0. Received: power={power}.")
    self.initial_learning_rate = float(initial_learning_rate)
    self.decay_steps = decay_steps
    self.end_learning_rate = float(end_learning_rate)
    self.power = float(power)
    self.cycle = bool(cycle)

  def __call__(self, step: int) -> float:
    s, ds = _F(step), _F(self.decay_steps)
    if self.cycle:
      ds = ds * (_F(1.0) if step == 0 else np.ceil(s / ds))
    else:
      s = np.minimum(s, ds)
    return float((_F(self.initial_learning_rate) - _F(self.end_learning_rate)) * np.power(_F(1.0) - s / ds, _F(self.power))
                 + _F(self.end_learning_rate))

  def get_config(self):
    return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                end_learning_rate=self.end_learning_rate, power=self.power, cycle=self.cycle)

  def min_value(self) -> float:
    # (1 - s / ds) ** power lies in [0, 1]: the value lies between the two ends
    return min(self.initial_learning_rate, self.end_learning_rate)

  def _device_description(self):
    return (KIND_POLYNOMIAL, [self.initial_learning_rate, float(self.decay_steps), self.end_learning_rate, self.power,
                              1.0 if self.cycle else 0.0], None)


class CosineDecay(LearningRateSchedule):
  """Without warm-up: ``s = min(step, decay_steps)``,
  ``lr = initial_learning_rate * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha)``.  With
  ``warmup_target``: for ``step < warmup_steps`` ``lr = initial + (warmup_target - initial) * step / warmup_steps``,
  then the cosine formula with ``warmup_target`` in place of ``initial_learning_rate`` and
  ``s = min(step - warmup_steps, decay_steps)``."""

  def __init__(self, initial_learning_rate: float, decay_steps: int, alpha: float = 0.0,
               warmup_target: Optional[float] = None, warmup_steps: int = 0):
    _check_decay_steps("CosineDecay", decay_steps)
    if warmup_target is not None and not warmup_steps > 0:
      raise ValueError(f"CosineDecay: `warmup_steps` must be > 0 with a `warmup_target`. Received: "
                       f"warmup_steps={warmup_steps}.")
    if warmup_steps < 0:
      raise ValueError(f"CosineDecay: `warmup_steps` must be >= 0. Received: warmup_steps={warmup_steps}.")
    self.initial_learning_rate = float(initial_learning_rate)
    self.decay_steps = decay_steps
    self.alpha = float(alpha)
    self.warmup_target = None if warmup_target is None else float(warmup_target)
    self.warmup_steps = warmup_steps

  def __call__(self, step: int) -> float:
    initial, s = _F(self.initial_learning_rate), _F(step)
    if self.warmup_target is not None:
      if step < self.warmup_steps:
        return float(initial + (_F(self.warmup_target) - initial) * s / _F(self.warmup_steps))
      initial, s = _F(self.warmup_target), s - _F(self.warmup_steps)
    s = np.minimum(s, _F(self.decay_steps))
    alpha = _F(self.alpha)
    return float(initial * ((_F(1.0) - alpha) * _F(0.5) * (_F(1.0) + np.cos(_F(np.pi) * s / _F(self.decay_steps))) + alpha))

  def get_config(self):
    return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps, alpha=self.alpha,
                warmup_target=self.warmup_target, warmup_steps=self.warmup_steps)

  def min_value(self) -> float:
    # the cosine factor lies between alpha and 1 (either order); the warm-up between initial and warmup_target
    peak = self.initial_learning_rate if self.warmup_target is None else self.warmup_target
    ends = [peak, peak * self.alpha]
    if self.warmup_target is not None:
      ends.append(self.initial_learning_rate)
    return min(ends)

  def _device_description(self):
    warm = self.warmup_target is not None
    return (KIND_COSINE, [self.initial_learning_rate, float(self.decay_steps), self.alpha, 1.0 if warm else 0.0,
                          self.warmup_target if warm else 0.0, float(self.warmup_steps)], None)


class PiecewiseConstantDecay(LearningRateSchedule):
  """``lr = values[i]`` for the smallest ``i`` with ``step <= boundaries[i]``, else ``values[-1]``.  Up to 7
  boundaries are compared on the device; more are expanded into a table of ``boundaries[-1] + 2`` values."""

  def __init__(self, boundaries: Sequence[float], values: Sequence[float]):
    boundaries, values = list(boundaries), [float(v) for v in values]
    if len(boundaries) != len(values) - 1:
      raise ValueError(f"The length of boundaries should be 1 less than the length of values. Received: "
                       f"boundaries={boundaries} of length {len(boundaries)}, and values={values} of length "
                       f"{len(values)}.")
    if not boundaries:
      raise ValueError("PiecewiseConstantDecay: at least one boundary")
    if any(b >= c for b, c in zip(boundaries, boundaries[1:])):
      raise ValueError(f"PiecewiseConstantDecay: boundaries must be strictly increasing. Received: {boundaries}.")
    if len(boundaries) > 7 and not 0 <= boundaries[-1] < _MAX_EXPANDED_TABLE - 2:
      raise ValueError(f"PiecewiseConstantDecay: more than 7 boundaries are expanded into a table, which needs the "
                       f"last boundary in [0, {_MAX_EXPANDED_TABLE - 2}). Received: {boundaries[-1]}.")
    self.boundaries = boundaries
    self.values = values

  def __call__(self, step: int) -> float:
    for b, v in zip(self.boundaries, self.values):
      if step <= b:
        return v
    return self.values[-1]

  def get_config(self):
    return dict(boundaries=list(self.boundaries), values=list(self.values))

  def min_value(self) -> float:
    return min(self.values)

  def _device_description(self):
    if len(self.boundaries) <= 7:
      return KIND_PIECEWISE, [float(b) for b in self.boundaries], np.asarray(self.values, dtype=np.float32)
    n = int(np.floor(self.boundaries[-1])) + 2
    return KIND_TABULATED, [], np.asarray([self(t) for t in range(n)], dtype=np.float32)


class Tabulated(LearningRateSchedule):
  """``lr = values[min(step, len(values) - 1)]``; the values are rounded to f32 once, on the host."""

  def __init__(self, values: Sequence[float]):
    table = np.asarray(values, dtype=np.float64).astype(np.float32)
    if table.ndim != 1 or table.size == 0:
      raise ValueError("Tabulated: `values` must be a non-empty 1-D sequence")
    self.values = table

  @classmethod
  def from_callable(cls, fn: Callable[[int], float], num_steps: int) -> "Tabulated":
    if not num_steps > 0:
      raise ValueError(f"Tabulated.from_callable: `num_steps` must be > 0. Received: num_steps={num_steps}.")
    return cls([float(fn(t)) for t in range(num_steps)])

  def __call__(self, step: int) -> float:
    return float(self.values[min(max(int(step), 0), self.values.size - 1)])

  def get_config(self):
    return dict(values=[float(v) for v in self.values])

  def min_value(self) -> float:
    return float(self.values.min())

  def _device_description(self):
    return KIND_TABULATED, [], self.values


_CLASSES = {cls.__name__: cls for cls in (ExponentialDecay, InverseTimeDecay, PolynomialDecay, CosineDecay,
                                          PiecewiseConstantDecay, Tabulated)}


def serialize(schedule: LearningRateSchedule) -> Dict[str, Any]:
  return {"class_name": type(schedule).__name__, "config": schedule.get_config()}


def deserialize(config: Dict[str, Any]) -> LearningRateSchedule:
  name = config.get("class_name") if isinstance(config, dict) else None
  if name not in _CLASSES:
    raise ValueError(f"unknown learning-rate schedule {name!r}; known: {sorted(_CLASSES)}")
  return _CLASSES[name].from_config(config["config"])
