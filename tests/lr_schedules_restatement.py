"""The learning-rate schedule formulas in NumPy float64, written from the formulas alone (not from
``recommenders_amd/schedules.py``): plain functions of the step, plus the single rounding to float32 that the device
floats hold.  ``step`` is the optimizer's ``iterations`` before the update (0 for the first step)."""

import numpy as np

f64 = np.float64


def f32(x) -> np.float32:
  """The one rounding of a float64 learning rate into the device float."""
  return np.float32(f64(x))


def ulps_apart(a: np.float32, b: np.float32) -> int:
  """Distance of two finite float32 of the same sign in units in the last place (0 = equal, 1 = adjacent)."""
  ia = int(np.array(a, dtype=np.float32).view(np.int32))
  ib = int(np.array(b, dtype=np.float32).view(np.int32))
  return abs(ia - ib)


def exponential_decay(step, initial, decay_steps, decay_rate, staircase=False):
  p = f64(step) / f64(decay_steps)
  if staircase:
    p = np.floor(p)
  return f64(initial) * np.power(f64(decay_rate), p)


def inverse_time_decay(step, initial, decay_steps, decay_rate, staircase=False):
  p = f64(step) / f64(decay_steps)
  if staircase:
    p = np.floor(p)
  return f64(initial) / (f64(1) + f64(decay_rate) * p)


def polynomial_decay(step, initial, decay_steps, end=1e-4, power=1.0, cycle=False):
  if cycle:
    s = f64(step)
    ds = f64(decay_steps) * (f64(1) if step == 0 else np.ceil(f64(step) / f64(decay_steps)))
  else:
    s = f64(min(step, decay_steps))
    ds = f64(decay_steps)
  return (f64(initial) - f64(end)) * np.power(f64(1) - s / ds, f64(power)) + f64(end)


def cosine_decay(step, initial, decay_steps, alpha=0.0, warmup_target=None, warmup_steps=0):
  if warmup_target is not None:
    if step < warmup_steps:
      return f64(initial) + (f64(warmup_target) - f64(initial)) * f64(step) / f64(warmup_steps)
    initial = warmup_target
    step = step - warmup_steps
  s = f64(min(step, decay_steps))
  return f64(initial) * ((f64(1) - f64(alpha)) * f64(0.5) * (f64(1) + np.cos(f64(np.pi) * s / f64(decay_steps))) + f64(alpha))


def piecewise_constant_decay(step, boundaries, values):
  assert len(values) == len(boundaries) + 1
  for i, b in enumerate(boundaries):
    if step <= b:
      return f64(values[i])
  return f64(values[-1])


def tabulated(step, values):
  """(values are rounded to float32 once, when the table is built)"""
  return f64(np.float32(values[min(step, len(values) - 1)]))
