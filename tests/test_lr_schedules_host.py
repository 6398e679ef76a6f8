"""Learning-rate schedules without a GPU: the host evaluation of every class of ``recommenders_amd/schedules.py``
against the independent float64 restatement (``tests/lr_schedules_restatement.py``) with ``==``, constructor errors,
configs, ``min_value``; the five optimizers on CPU tensors under a schedule against the same optimizer whose float
learning rate is set by hand before every step; the argument checks of the new C entries (before any device call)."""

import ctypes

import numpy as np
import pytest
import torch

from recommenders_amd import optimizers, schedules
from recommenders_amd.experimental.optimizers import ClippyAdagrad
from recommenders_amd.optimizers import Adagrad, Adam, Ftrl, SGD
from tests import lr_schedules_restatement as rs

DS = 10     # decay_steps of the closed forms below


def _steps(ds=DS):
  return [0, 1, ds - 1, ds, ds + 1, 3 * ds + 2]


# (schedule, restatement as a function of the step, the steps)
def _cases():
  S = schedules
  out = []
  for staircase in (False, True):
    out.append((S.ExponentialDecay(0.1, DS, 0.5, staircase=staircase),
                lambda t, st=staircase: rs.exponential_decay(t, 0.1, DS, 0.5, st), _steps()))
    out.append((S.InverseTimeDecay(0.1, DS, 0.5, staircase=staircase),
                lambda t, st=staircase: rs.inverse_time_decay(t, 0.1, DS, 0.5, st), _steps()))
  for cycle in (False, True):
    for power in (1.0, 2.0):
      out.append((S.PolynomialDecay(0.5, DS, 0.05, power=power, cycle=cycle),
                  lambda t, c=cycle, p=power: rs.polynomial_decay(t, 0.5, DS, 0.05, p, c), _steps()))
  for alpha in (0.0, 0.1):
    out.append((S.CosineDecay(0.3, DS, alpha=alpha), lambda t, a=alpha: rs.cosine_decay(t, 0.3, DS, a), _steps()))
    out.append((S.CosineDecay(0.01, DS, alpha=alpha, warmup_target=0.3, warmup_steps=4),
                lambda t, a=alpha: rs.cosine_decay(t, 0.01, DS, a, 0.3, 4), _steps() + [3, 4, 5, DS + 3, DS + 4, DS + 5]))
  one = ([5], [0.5, 0.1])
  seven = ([2, 4, 7, 11, 12, 20, 33], [0.5, 0.4, 0.3, 0.25, 0.2, 0.1, 0.05, 0.01])
  for boundaries, values in (one, seven):
    steps = sorted({0, 1} | {b for b in boundaries} | {b + 1 for b in boundaries} | {3 * boundaries[-1] + 2})
    out.append((S.PiecewiseConstantDecay(boundaries, values),
                lambda t, b=boundaries, v=values: rs.piecewise_constant_decay(t, b, v), steps))
  table = [0.5, 0.25, 0.125, 0.1, 1.0 / 3.0]
  out.append((S.Tabulated(table), lambda t, v=table: rs.tabulated(t, v), [0, 1, 3, 4, 5, 17]))
  out.append((S.Tabulated.from_callable(lambda t: 0.3 / (1.0 + t), 6),
              lambda t: rs.tabulated(t, [0.3 / (1.0 + i) for i in range(6)]), [0, 1, 5, 6, 20]))
  return out


@pytest.mark.parametrize("index", range(len(_cases())))
def test_host_formulas_equal_the_restatement(index):
  schedule, restated, steps = _cases()[index]
  for t in steps:
    got = schedule(t)
    assert isinstance(got, float)
    assert got == float(restated(t)), (type(schedule).__name__, schedule.get_config(), t, got, float(restated(t)))


def test_piecewise_with_more_than_seven_boundaries_goes_through_the_table():
  boundaries = [1, 3, 4, 8, 9, 12, 13, 20, 22]
  values = [0.1 * (i + 1) for i in range(10)]
  s = schedules.PiecewiseConstantDecay(boundaries, values)
  kind, params, table = s._device_description()
  assert kind == schedules.KIND_TABULATED and table.dtype == np.float32 and table.size == boundaries[-1] + 2
  for t in range(0, 40):
    assert s(t) == float(rs.piecewise_constant_decay(t, boundaries, values))
    assert table[min(t, table.size - 1)] == rs.f32(rs.piecewise_constant_decay(t, boundaries, values))
  kind, params, table = schedules.PiecewiseConstantDecay(boundaries[:7], values[:8])._device_description()
  assert kind == schedules.KIND_PIECEWISE and len(params) == 7 and table.size == 8


def test_constructor_errors():
  S = schedules
  for cls in (S.ExponentialDecay, S.InverseTimeDecay):
    with pytest.raises(ValueError, match="decay_steps"):
      cls(0.1, 0, 0.5)
    with pytest.raises(ValueError, match="decay_steps"):
      cls(0.1, -3, 0.5)
  with pytest.raises(ValueError, match="decay_steps"):
    S.PolynomialDecay(0.1, 0)
  with pytest.raises(ValueError, match="decay_steps"):
    S.CosineDecay(0.1, 0)
  with pytest.raises(ValueError, match="warmup_steps"):
    S.CosineDecay(0.1, 10, warmup_target=0.5, warmup_steps=0)
  with pytest.raises(ValueError, match="1 less"):
    S.PiecewiseConstantDecay([1, 2], [0.1, 0.2])
  with pytest.raises(ValueError, match="increasing"):
    S.PiecewiseConstantDecay([3, 2], [0.1, 0.2, 0.3])
  with pytest.raises(ValueError):
    S.Tabulated([])
  with pytest.raises(ValueError, match="num_steps"):
    S.Tabulated.from_callable(lambda t: 0.1, 0)
  with pytest.raises(ValueError, match="unknown learning-rate schedule"):
    S.deserialize({"class_name": "CosineDecayRestarts", "config": {}})


@pytest.mark.parametrize("index", range(len(_cases())))
def test_config_round_trip_and_min_value(index):
  schedule, _, steps = _cases()[index]
  config = schedules.serialize(schedule)
  assert set(config) == {"class_name", "config"} and config["class_name"] == type(schedule).__name__
  again = schedules.deserialize(config)
  assert type(again) is type(schedule)
  assert schedules.serialize(again) == config
  assert type(schedule).from_config(schedule.get_config()).get_config() == schedule.get_config()
  for t in steps:
    assert again(t) == schedule(t)
  ds = getattr(schedule, "decay_steps", DS)
  assert schedule.min_value() <= min(schedule(t) for t in range(4 * ds))


def test_schedules_module_is_reachable_from_optimizers():
  import recommenders_amd
  assert optimizers.schedules is schedules is recommenders_amd.schedules
  assert issubclass(schedules.CosineDecay, schedules.LearningRateSchedule)


# ---- the optimizers on CPU tensors ---------------------------------------------------------------------------------
_OPTIMIZERS = {
    "Adagrad": (Adagrad, {}),
    "SGD": (SGD, {}),
    "Adam": (Adam, {}),
    "Ftrl": (Ftrl, dict(l1_regularization_strength=0.001, l2_regularization_strength=0.01, beta=0.1)),
    "ClippyAdagrad": (ClippyAdagrad, {}),
}
_BOUNDARY = ([2], [0.5, 0.125])      # steps 0, 1, 2 at 0.5; from step 3 on 0.125


def _cpu_gradients(steps):
  g = torch.Generator().manual_seed(11)
  return [(torch.randn(6, 4, generator=g), torch.randn(3, generator=g)) for _ in range(steps)]


def _cpu_parameters():
  g = torch.Generator().manual_seed(12)
  return [torch.nn.Parameter(torch.randn(6, 4, generator=g)), torch.nn.Parameter(torch.randn(3, generator=g))]


def _run_cpu(opt, params, grads, by_hand=None, first_step=0):
  for t, (ga, gb) in enumerate(grads, start=first_step):
    if by_hand is not None:
      for group in opt.param_groups:
        group["learning_rate"] = float(np.float32(by_hand(t)))
    params[0].grad, params[1].grad = ga.clone(), gb.clone()
    opt.step()


def _assert_same_state(params_a, opt_a, params_b, opt_b):
  for pa, pb in zip(params_a, params_b):
    assert torch.equal(pa, pb)
    for key, value in opt_b.state[pb].items():     # every slot of the float-path optimizer
      assert torch.equal(opt_a.state[pa][key], value), key


@pytest.mark.parametrize("name", sorted(_OPTIMIZERS))
def test_cpu_optimizer_under_a_schedule_equals_the_float_path_set_by_hand(name):
  cls, kwargs = _OPTIMIZERS[name]
  schedule = schedules.PiecewiseConstantDecay(*_BOUNDARY)
  grads = _cpu_gradients(9)
  ps, pf = _cpu_parameters(), _cpu_parameters()
  scheduled = cls(ps, learning_rate=schedule, **kwargs)
  by_float = cls(pf, learning_rate=0.5, **kwargs)
  assert int(scheduled.iterations) == 0                      # the counter exists from the constructor on
  _run_cpu(scheduled, ps, grads[:6])
  _run_cpu(by_float, pf, grads[:6], by_hand=schedule)
  assert isinstance(scheduled.iterations, torch.Tensor) and scheduled.iterations.dtype == torch.int64
  assert int(scheduled.iterations) == 6
  _assert_same_state(ps, scheduled, pf, by_float)
  # a float learning rate keeps its state_dict: no counter, no device float
  keys = {k for st in by_float.state_dict()["state"].values() for k in st}
  assert "iterations" not in keys and "learning_rate" not in keys
  # state_dict -> fresh optimizer -> load_state_dict continues the schedule at step 6
  saved = scheduled.state_dict()
  pr = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  resumed = cls(pr, learning_rate=schedules.PiecewiseConstantDecay(*_BOUNDARY), **kwargs)
  resumed.load_state_dict(saved)
  assert resumed.iterations.dtype == torch.int64 and int(resumed.iterations) == 6
  _run_cpu(resumed, pr, grads[6:])
  _run_cpu(by_float, pf, grads[6:], by_hand=schedule, first_step=6)
  assert int(resumed.iterations) == 9
  _assert_same_state(pr, resumed, pf, by_float)
  # reset_state_ zeroes the counter
  resumed.reset_state_()
  assert int(resumed.iterations) == 0
  # config round trip
  config = scheduled.get_config()
  assert config["learning_rate"] == schedules.serialize(schedule)
  again = cls.from_config(_cpu_parameters(), config)
  assert isinstance(again.param_groups[0]["learning_rate"], schedules.PiecewiseConstantDecay)
  assert again.get_config() == config


def test_cpu_learning_rate_tensor_and_callable_forms():
  """A 0-d float32 tensor (or a zero-argument callable returning one, called once) is read at every step."""
  grads = _cpu_gradients(4)
  lr = torch.tensor(0.5)
  calls = []

  def make():
    calls.append(1)
    return lr

  pt, pf = _cpu_parameters(), _cpu_parameters()
  by_tensor, by_float = SGD(pt, learning_rate=make), SGD(pf, learning_rate=0.5)
  assert by_tensor.param_groups[0]["learning_rate"] is lr
  _run_cpu(by_tensor, pt, grads[:2])
  _run_cpu(by_float, pf, grads[:2])
  lr.fill_(0.05)
  by_float.param_groups[0]["learning_rate"] = float(np.float32(0.05))
  _run_cpu(by_tensor, pt, grads[2:])
  _run_cpu(by_float, pf, grads[2:])
  assert len(calls) == 1 and int(by_tensor.iterations) == 4
  _assert_same_state(pt, by_tensor, pf, by_float)
  with pytest.raises(ValueError, match="0-d float32"):
    SGD(_cpu_parameters(), learning_rate=torch.zeros(2))
  with pytest.raises(ValueError, match="0-d float32"):
    Adagrad(_cpu_parameters(), learning_rate=torch.tensor(0.5, dtype=torch.float64))
  with pytest.raises(ValueError, match="callable must return"):
    Adagrad(_cpu_parameters(), learning_rate=lambda: 0.5)


def test_ftrl_refuses_a_schedule_that_reaches_zero():
  with pytest.raises(ValueError, match="positive"):
    Ftrl(_cpu_parameters(), learning_rate=schedules.PolynomialDecay(0.1, 10, end_learning_rate=0.0))
  with pytest.raises(ValueError, match="positive"):
    Ftrl(_cpu_parameters(), learning_rate=schedules.CosineDecay(0.1, 10))      # alpha = 0: ends at 0
  Ftrl(_cpu_parameters(), learning_rate=schedules.ExponentialDecay(0.1, 4, 0.5))   # approaches 0, never reaches it
  Ftrl(_cpu_parameters(), learning_rate=schedules.CosineDecay(0.1, 10, alpha=0.1))


# ---- the C entries: every argument check comes before any device call ----------------------------------------------
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


def test_argument_validation_of_the_tick_entries_without_gpu(lib):
  from recommenders_amd import _lib
  params = (ctypes.c_double * 8)(0.1, 10.0, 0.5, 0.0)
  fake = ctypes.c_void_p(256)     # never dereferenced: every call below fails its checks first
  # NULL counter / NULL output
  assert lib.tfrs_lr_tick(None, fake, 1, params, None, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  assert "lr_tick" in _lib.last_error() and "NULL" in _lib.last_error()
  assert lib.tfrs_lr_tick(fake, None, 1, params, None, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  # unknown kind
  for kind in (-1, 7, 99):
    assert lib.tfrs_lr_tick(fake, fake, kind, params, None, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
    assert "unknown schedule kind" in _lib.last_error()
  # the table kinds (0 external, 5 piecewise, 6 tabulated) without a table, or with an empty one
  for kind in (schedules.KIND_EXTERNAL, schedules.KIND_PIECEWISE, schedules.KIND_TABULATED):
    assert lib.tfrs_lr_tick(fake, fake, kind, params, None, 4, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
    assert "needs a device table" in _lib.last_error()
    assert lib.tfrs_lr_tick(fake, fake, kind, params, fake, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  # a piecewise schedule compares at most 7 boundaries
  assert lib.tfrs_lr_tick(fake, fake, schedules.KIND_PIECEWISE, params, fake, 9, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_lr_tick(fake, fake, schedules.KIND_PIECEWISE, params, fake, 1, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  # NULL parameters, decay_steps <= 0, advance, Ftrl's terms
  assert lib.tfrs_lr_tick(fake, fake, 1, None, None, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  bad = (ctypes.c_double * 8)(0.1, 0.0, 0.5, 0.0)
  for kind in (1, 2, 3, 4):
    assert lib.tfrs_lr_tick(fake, fake, kind, bad, None, 0, 0, 0.0, 0.0, 1, None) == _lib.TFRS_EINVAL
    assert "decay_steps" in _lib.last_error()
  assert lib.tfrs_lr_tick(fake, fake, 1, params, None, 0, 0, 0.0, 0.0, 2, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_lr_tick(fake, fake, 1, params, None, 0, 1, -1.0, 0.0, 1, None) == _lib.TFRS_EINVAL
  with pytest.raises(ValueError, match="lr_tick"):
    _lib.check(lib.tfrs_lr_tick(None, None, 1, params, None, 0, 0, 0.0, 0.0, 1, None))
  # Adam's tick with a schedule
  tick = lib.tfrs_adam_tick_scheduled
  assert tick(None, fake, fake, 1, params, None, 0, 0.9, 0.999, 1, None) == _lib.TFRS_EINVAL
  assert tick(fake, fake, None, 1, params, None, 0, 0.9, 0.999, 1, None) == _lib.TFRS_EINVAL
  assert tick(fake, fake, fake, 42, params, None, 0, 0.9, 0.999, 1, None) == _lib.TFRS_EINVAL
  assert "unknown schedule kind" in _lib.last_error()
  assert tick(fake, fake, fake, schedules.KIND_TABULATED, params, None, 3, 0.9, 0.999, 1, None) == _lib.TFRS_EINVAL
  assert tick(fake, fake, fake, 1, params, None, 0, 1.0, 0.999, 1, None) == _lib.TFRS_EINVAL
  # the device-lr variants keep the checks of the entries that forward to them
  f = ctypes.c_float
  assert lib.tfrs_adagrad_dense_multi_dlr(0, None, None, None, None, f(0.1), fake, f(1e-7), 1, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_clippy_dense_multi_dlr(1, None, None, None, None, None, f(0.1), fake, f(1e-7), f(0.1), f(0.0),
                                         f(1e-7), 0, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_embedding_scatter_add_rowscan_dlr(None, None, 1, 4, 300, 10, fake, fake, f(0.1), fake, f(1e-7), 1,
                                                    None) == _lib.TFRS_EINVAL
  assert lib.tfrs_embedding_scatter_add_unsorted_dlr(None, None, 1, 4, 0, 10, fake, fake, f(0.1), fake, f(1e-7), 1,
                                                     None, 0, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_clippy_sparse_dlr(None, None, 1, 4, 8, 10, None, None, None, f(0.1), fake, f(1e-7), f(0.1), f(0.0),
                                    f(1e-7), 0, 1, None, 0, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_embedding_scatter_add_rowscan_multi_dlr(0, None, None, None, None, None, None, None, None, f(0.1),
                                                          fake, f(1e-7), 1, None) == _lib.TFRS_EINVAL
