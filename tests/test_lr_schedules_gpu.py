"""Learning-rate schedules on the device: the tick kernel against the float64 restatement rounded to f32
(``tests/lr_schedules_restatement.py``), the device-lr instantiations of every update kernel against the constant-lr
kernels bit for bit, and ``Model.fit`` replaying ONE captured step through a whole schedule."""

import ctypes

import numpy as np
import pytest
import torch

from recommenders_amd import schedules
from tests import lr_schedules_restatement as rs

pytestmark = pytest.mark.gpu

DS = 10


def _np(t):
  return t.detach().cpu().numpy()


# ---- the tick kernel -----------------------------------------------------------------------------------------------
def _tick_cases():
  S = schedules
  table = [0.5, 0.25, 0.125, 0.1, 1.0 / 3.0, 0.3, 0.2]
  seven = ([2, 4, 7, 11, 12, 20, 33], [0.5, 0.4, 0.3, 0.25, 0.2, 0.1, 0.05, 0.01])
  nine = ([1, 3, 4, 8, 9, 12, 13, 20, 22], [0.1 * (i + 1) for i in range(10)])
  # (name, schedule, restatement, exact)
  return [
      ("exponential", S.ExponentialDecay(0.1, DS, 0.5), lambda t: rs.exponential_decay(t, 0.1, DS, 0.5), False),
      ("exponential_staircase", S.ExponentialDecay(0.1, DS, 0.5, True), lambda t: rs.exponential_decay(t, 0.1, DS, 0.5, True), False),
      ("inverse_time", S.InverseTimeDecay(0.1, DS, 0.5), lambda t: rs.inverse_time_decay(t, 0.1, DS, 0.5), False),
      ("inverse_time_staircase", S.InverseTimeDecay(0.1, DS, 0.5, True), lambda t: rs.inverse_time_decay(t, 0.1, DS, 0.5, True), False),
      ("polynomial", S.PolynomialDecay(0.5, DS, 0.05), lambda t: rs.polynomial_decay(t, 0.5, DS, 0.05), False),
      ("polynomial_square_cycle", S.PolynomialDecay(0.5, DS, 0.05, power=2.0, cycle=True),
       lambda t: rs.polynomial_decay(t, 0.5, DS, 0.05, 2.0, True), False),
      ("polynomial_long", S.PolynomialDecay(0.5, 10**4, 0.05, power=0.5), lambda t: rs.polynomial_decay(t, 0.5, 10**4, 0.05, 0.5), False),
      ("cosine", S.CosineDecay(0.3, DS), lambda t: rs.cosine_decay(t, 0.3, DS), False),
      ("cosine_alpha_warmup", S.CosineDecay(0.01, DS, alpha=0.1, warmup_target=0.3, warmup_steps=4),
       lambda t: rs.cosine_decay(t, 0.01, DS, 0.1, 0.3, 4), False),
      ("cosine_long", S.CosineDecay(0.3, 10**4), lambda t: rs.cosine_decay(t, 0.3, 10**4), False),
      ("piecewise_1", S.PiecewiseConstantDecay([9], [0.5, 0.1]), lambda t: rs.piecewise_constant_decay(t, [9], [0.5, 0.1]), True),
      ("piecewise_7", S.PiecewiseConstantDecay(*seven), lambda t: rs.piecewise_constant_decay(t, *seven), True),
      ("piecewise_9_through_the_table", S.PiecewiseConstantDecay(*nine), lambda t: rs.piecewise_constant_decay(t, *nine), True),
      ("tabulated", S.Tabulated(table), lambda t: rs.tabulated(t, table), True),
  ]


def _ticks(schedule, start: int, count: int, ftrl=None):
  """``count`` consecutive ``tfrs_lr_tick`` calls from ``iterations = start``: the floats written and the counter."""
  from recommenders_amd import _lib
  from recommenders_amd.optimizers import SliceOwningOptimizer
  lib = _lib.load()
  device = torch.device("cuda")
  counter = torch.full((), start, dtype=torch.int64, device=device)
  out = torch.zeros((count, 2), dtype=torch.float32, device=device)
  kind, params, table, table_len = SliceOwningOptimizer._schedule_args(schedule, device)
  for i in range(count):
    _lib.check(lib.tfrs_lr_tick(_lib.ptr(counter), ctypes.c_void_p(out.data_ptr() + 8 * i), kind, params,
                                _lib.ptr(table), table_len, 0 if ftrl is None else 1, *(ftrl or (0.0, 0.0)), 1,
                                _lib.current_stream()))
  return _np(out), int(counter)


@pytest.mark.parametrize("case", _tick_cases(), ids=lambda c: c[0])
def test_tick_kernel_follows_the_restatement(case):
  """64 consecutive ticks from 0 and from ``decay_steps - 2``.  The table kinds copy an f32: equal.  The closed forms
  are evaluated in float64 on both sides -- the device's pow / cos are accurate to a few double ulps, 29 bits below an
  f32 ulp -- and rounded once: equal or adjacent float32 (1 ulp), adjacent only at a rounding boundary."""
  name, schedule, restated, exact = case
  ds = getattr(schedule, "decay_steps", DS)
  for start in (0, ds - 2):
    got, counter = _ticks(schedule, start, 64)
    assert counter == start + 64
    worst = 0
    for i in range(64):
      want = rs.f32(restated(start + i))
      apart = rs.ulps_apart(got[i, 0], want)
      worst = max(worst, apart)
      assert apart <= (0 if exact else 1), (name, start + i, got[i, 0], want)
    print(f"{name} from {start}: worst distance {worst} ulp")


def test_tick_kernel_writes_ftrl_term_and_advance_zero_keeps_the_counter():
  from recommenders_amd import _lib
  from recommenders_amd.optimizers import SliceOwningOptimizer
  schedule = schedules.Tabulated([0.5, 0.25, 0.1])
  got, counter = _ticks(schedule, 0, 4, ftrl=(0.01, 0.1))
  assert counter == 4
  for i in range(4):
    lr = np.float32(schedule(i))
    assert got[i, 0] == lr
    assert got[i, 1] == np.float32(2.0 * (0.01 + 0.1 / (2.0 * float(lr))))
  # advance == 0: evaluated at the same t, the counter stays
  lib = _lib.load()
  counter = torch.full((), 2, dtype=torch.int64, device="cuda")
  out = torch.zeros((2,), dtype=torch.float32, device="cuda")
  kind, params, table, table_len = SliceOwningOptimizer._schedule_args(schedule, out.device)
  _lib.check(lib.tfrs_lr_tick(_lib.ptr(counter), _lib.ptr(out), kind, params, _lib.ptr(table), table_len, 0, 0.0, 0.0,
                              0, _lib.current_stream()))
  assert int(counter) == 2 and float(out[0]) == float(np.float32(0.1))


@pytest.mark.parametrize("name", ["Adagrad", "SGD", "Adam", "Ftrl", "ClippyAdagrad"])
def test_two_groups_are_evaluated_at_the_same_step_and_the_counter_advances_once(name):
  cls, kwargs = _optimizer(name)
  a = torch.nn.Parameter(torch.randn(5, 3, device="cuda"))
  b = torch.nn.Parameter(torch.randn(7, device="cuda"))
  sa, sb = schedules.ExponentialDecay(0.1, 4, 0.5), schedules.PolynomialDecay(0.5, 6, 0.05)
  opt = cls([dict(params=[a], learning_rate=sa), dict(params=[b], learning_rate=sb)], **kwargs)
  assert int(opt.iterations) == 0
  for t in range(3):
    a.grad, b.grad = torch.randn_like(a), torch.randn_like(b)
    opt.step()
    assert int(opt.iterations) == t + 1
    la, lb = (np.float32(float(opt.state[p]["learning_rate"][0])) for p in (a, b))
    assert rs.ulps_apart(la, rs.f32(rs.exponential_decay(t, 0.1, 4, 0.5))) <= 1
    assert rs.ulps_apart(lb, rs.f32(rs.polynomial_decay(t, 0.5, 6, 0.05))) <= 1


# ---- the scheduled kernels against the float kernels, bit for bit --------------------------------------------------
def _optimizer(name):
  from recommenders_amd import optimizers
  from recommenders_amd.experimental.optimizers import ClippyAdagrad
  return {
      "Adagrad": (optimizers.Adagrad, {}),
      "SGD": (optimizers.SGD, {}),
      "Adam": (optimizers.Adam, {}),
      "Ftrl": (optimizers.Ftrl, dict(l1_regularization_strength=0.001, l2_regularization_strength=0.01, beta=0.1)),
      "ClippyAdagrad": (ClippyAdagrad, dict(export_clipping_factors=True)),
  }[name]


def _table(vocab, d, gen):
  p = torch.nn.Parameter((torch.randn(vocab, d, generator=gen) * 0.05).cuda())
  p._tfrs_embedding = True
  return p


def _route(route, gen):
  """``(tables, dense parameters, ids per table)`` of a route of the update kernels, at the smallest shapes that reach
  it (``layers.embedding._use_rowscan``: the row scan while vocab * n <= 2^26)."""
  from recommenders_amd.layers import embedding as emb
  if route == "rowscan":
    ids = torch.randint(0, 50, (40,), generator=gen)
    ids[3], ids[17], ids[29] = ids[0], ids[0], 57        # duplicates, and one id outside the vocabulary
    assert emb._use_rowscan(50, 40, 8)
    return [_table(50, 8, gen)], [], [ids]
  if route in ("sorted_d8", "sorted_d6"):
    d = 8 if route == "sorted_d8" else 6
    ids = torch.randint(0, 70_000, (1024,), generator=gen)
    ids[100:140] = 12_345                                # a run of 40: longer than a piece of 32 positions
    ids = ids[torch.randperm(1024, generator=gen)]
    assert not emb._use_rowscan(70_000, 1024, d)
    return [_table(70_000, d, gen)], [], [ids]
  if route == "rowscan_multi":
    return ([_table(50, 8, gen), _table(31, 6, gen)], [],
            [torch.randint(0, 50, (40,), generator=gen), torch.randint(0, 31, (24,), generator=gen)])
  if route == "dense":
    return [], [torch.nn.Parameter(torch.randn(33, 7, generator=gen).cuda()), torch.nn.Parameter(torch.randn(5, generator=gen).cuda())], []
  assert route == "dense_33"                              # a second launch of 32 + 1 tensors
  return [], [torch.nn.Parameter(torch.randn(3 + i % 4, generator=gen).cuda()) for i in range(33)], []


@pytest.mark.parametrize("route", ["rowscan", "sorted_d8", "sorted_d6", "rowscan_multi", "dense", "dense_33"])
@pytest.mark.parametrize("name", ["Adagrad", "SGD", "Adam", "Ftrl", "ClippyAdagrad"])
def test_scheduled_kernels_have_the_bits_of_the_float_kernels(name, route):
  """Six steps under ``ExponentialDecay(0.1, 4, 0.5)`` against a twin on the float path whose learning rate is set,
  before each step, to the f32 the scheduled optimizer's device float held: parameters and every slot equal."""
  cls, kwargs = _optimizer(name)
  scale = 50.0 if name == "ClippyAdagrad" else 1.0       # large enough that ClippyAdagrad clips (asserted below)
  tables_s, dense_s, ids = _route(route, torch.Generator().manual_seed(3))
  tables_f, dense_f, _ = _route(route, torch.Generator().manual_seed(3))
  ids = [i.cuda() for i in ids]
  scheduled = cls(tables_s + dense_s, learning_rate=schedules.ExponentialDecay(0.1, 4, 0.5), **kwargs)
  by_float = cls(tables_f + dense_f, learning_rate=0.1, **kwargs)
  first = (tables_s + dense_s)[0]
  gen = torch.Generator().manual_seed(4)
  clipped = False
  for t in range(6):
    rows = [(torch.randn(i.numel(), p.shape[1], generator=gen) * scale).cuda() for i, p in zip(ids, tables_s)]
    grads = [(torch.randn(p.shape, generator=gen) * scale).cuda() for p in dense_s]
    for tables, dense in ((tables_s, dense_s), (tables_f, dense_f)):
      for p, i, r in zip(tables, ids, rows):
        p._tfrs_slices.append((i, r))
      for p, g in zip(dense, grads):
        p.grad = g.clone()
    scheduled.step()
    lr = float(scheduled.state[first]["learning_rate"][0])
    assert rs.ulps_apart(np.float32(lr), rs.f32(rs.exponential_decay(t, 0.1, 4, 0.5))) <= 1, (t, lr)
    for group in by_float.param_groups:
      group["learning_rate"] = lr
    by_float.step()
    if name == "ClippyAdagrad":
      fs, ff = torch.stack(scheduled.clipping_factors), torch.stack(by_float.clipping_factors)
      assert torch.equal(fs, ff)
      clipped = clipped or bool((fs < 1.0).any())
  assert int(scheduled.iterations) == 6
  assert name != "ClippyAdagrad" or clipped
  for ps, pf in zip(tables_s + dense_s, tables_f + dense_f):
    assert torch.equal(ps, pf)
    slots = {k: v for k, v in by_float.state[pf].items() if k not in ("step", "alpha")}
    assert slots or name == "SGD"
    for key, value in slots.items():
      assert torch.equal(scheduled.state[ps][key], value), key
  scheduled.close()
  by_float.close()


# ---- Model.fit: one captured step replays the whole schedule -------------------------------------------------------
def _batches(rng, sizes):
  return [{"user_id": torch.as_tensor(rng.integers(0, 943, size=n)).cuda(),
           "movie_id": torch.as_tensor(rng.integers(0, 1682, size=n)).cuda()} for n in sizes]


def _quickstart(tfrs, make_optimizer, with_metrics=False, seed=5):
  """The README quickstart two-tower model at the MovieLens-100K shapes (as the fit tests of test_ops_gpu.py build it)."""

  class TwoTower(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.user_model = tfrs.layers.embedding.Embedding(943, 64)
      self.item_model = tfrs.layers.embedding.Embedding(1682, 64)
      if with_metrics:
        movies = tfrs.data.Dataset.from_tensor_slices(torch.arange(1682, device="cuda"))
        self.task = tfrs.tasks.Retrieval(metrics=tfrs.metrics.FactorizedTopK(
            candidates=movies.batch(128).map(self.item_model)))
      else:
        self.task = tfrs.tasks.Retrieval()

    def compute_loss(self, features, training=False):
      return self.task(self.user_model(features["user_id"]), self.item_model(features["movie_id"]),
                       compute_metrics=with_metrics)

  torch.manual_seed(seed)
  m = TwoTower()
  m.compile(optimizer=make_optimizer(m))
  return m


def _assert_same_model(eager, graphed):
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a), _np(b))
  for (pa, sa), (pb, sb) in zip(eager.optimizer.state.items(), graphed.optimizer.state.items()):
    assert set(sa) == set(sb)
    for key in sa:
      if isinstance(sa[key], torch.Tensor):
        np.testing.assert_array_equal(_np(sa[key]), _np(sb[key]), err_msg=key)


def _captured(model):
  return sum(callable(v) for v in model.__dict__.get("_fit_graphs", {}).values())


def test_fit_replays_one_captured_step_through_a_schedule():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(31)
  batches = _batches(rng, [512] * 4)
  make = lambda m: tfrs.optimizers.Adagrad(m.parameters(), learning_rate=schedules.PolynomialDecay(0.5, 6, 0.05))
  eager, graphed = _quickstart(tfrs, make, with_metrics=True), _quickstart(tfrs, make, with_metrics=True)
  assert graphed._graph_steps_allowed(None, training=True)
  he = eager.fit(batches, epochs=1, graph=False)
  hg = graphed.fit(batches, epochs=1)
  cache = graphed.__dict__["_fit_graphs"]
  assert _captured(graphed) == 1 and "_errors" not in cache
  he2 = eager.fit(batches, epochs=1, graph=False)
  hg2 = graphed.fit(batches, epochs=1)
  assert graphed.__dict__["_fit_graphs"] is cache and _captured(graphed) == 1      # nothing dropped, nothing re-captured
  assert he == hg and he2 == hg2
  # the counter counts the steps taken: the capture's warm-up iterations were rolled back
  assert int(eager.optimizer.iterations) == 8 and int(graphed.optimizer.iterations) == 8
  _assert_same_model(eager, graphed)
  # ... and the learning rate the last step used is the schedule's value at step 7
  lr = float(graphed.optimizer.state[next(graphed.parameters())]["learning_rate"][0])
  assert rs.ulps_apart(np.float32(lr), rs.f32(rs.polynomial_decay(7, 0.5, 6, 0.05))) <= 1
  # the same in one call of two epochs
  eager2, graphed2 = _quickstart(tfrs, make, with_metrics=True), _quickstart(tfrs, make, with_metrics=True)
  assert eager2.fit(batches, epochs=2, graph=False) == graphed2.fit(batches, epochs=2)
  assert _captured(graphed2) == 1 and int(graphed2.optimizer.iterations) == 8
  _assert_same_model(eager2, graphed2)
  _assert_same_model(eager, eager2)


def test_fit_replays_a_composite_of_scheduled_adagrad_and_scheduled_adam():
  import recommenders_amd as tfrs
  from recommenders_amd.experimental.optimizers import CompositeOptimizer

  class Tower(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.users = tfrs.layers.embedding.Embedding(943, 32)
      self.items = tfrs.layers.embedding.Embedding(1682, 32)
      self.mlp = tfrs.layers.blocks.MLP([16, 1])

    def compute_loss(self, inputs, training=False):
      x = torch.cat([self.users(inputs["user_id"]), self.items(inputs["movie_id"])], dim=-1)
      return (self.mlp(x).squeeze(-1) - 1.0).square().mean()

  def build():
    torch.manual_seed(77)
    model = Tower().cuda()
    with torch.no_grad():      # (builds the lazily created MLP kernels)
      model.compute_loss({"user_id": torch.zeros(8, dtype=torch.int64, device="cuda"),
                          "movie_id": torch.zeros(8, dtype=torch.int64, device="cuda")})
    tables = [model.users.embeddings, model.items.embeddings]
    dense = [p for p in model.parameters() if all(p is not t for t in tables)]
    adagrad = tfrs.optimizers.Adagrad(tables, learning_rate=schedules.PolynomialDecay(0.5, 6, 0.05))
    adam = tfrs.optimizers.Adam(dense, learning_rate=schedules.CosineDecay(0.001, 5, alpha=0.1, warmup_target=0.01,
                                                                           warmup_steps=3))
    model.compile(optimizer=CompositeOptimizer([(adagrad, lambda: tables), (adam, lambda: dense)]))
    return model, adagrad, adam

  rng = np.random.default_rng(32)
  batches = _batches(rng, [512] * 4)
  (eager, _, _), (graphed, adagrad, adam) = build(), build()
  assert graphed._graph_steps_allowed(None, training=True)
  he = eager.fit(batches, epochs=2, graph=False)
  hg = graphed.fit(batches, epochs=2)
  assert he == hg
  assert _captured(graphed) == 1 and "_errors" not in graphed.__dict__["_fit_graphs"]
  assert int(adagrad.iterations) == 8 and int(adam.iterations) == 8
  _assert_same_model(eager, graphed)


def test_replacing_the_schedule_or_switching_to_a_float_drops_the_captured_steps():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(33)
  batches = _batches(rng, [512] * 3)
  make = lambda m: tfrs.optimizers.Adagrad(m.parameters(), learning_rate=schedules.PolynomialDecay(0.5, 6, 0.05))
  eager, graphed = _quickstart(tfrs, make), _quickstart(tfrs, make)
  assert eager.fit(batches, epochs=2, graph=False) == graphed.fit(batches, epochs=2)
  cache = graphed.__dict__["_fit_graphs"]
  assert _captured(graphed) == 1
  for m in (eager, graphed):      # another schedule object (continuing at the optimizer's counter)
    for group in m.optimizer.param_groups:
      group["learning_rate"] = schedules.ExponentialDecay(0.3, 4, 0.5)
  assert eager.fit(batches, epochs=2, graph=False) == graphed.fit(batches, epochs=2)
  assert graphed.__dict__["_fit_graphs"] is not cache and _captured(graphed) == 1
  _assert_same_model(eager, graphed)
  cache = graphed.__dict__["_fit_graphs"]
  for m in (eager, graphed):      # ... and a float
    for group in m.optimizer.param_groups:
      group["learning_rate"] = 0.05
  assert eager.fit(batches, epochs=2, graph=False) == graphed.fit(batches, epochs=2)
  assert graphed.__dict__["_fit_graphs"] is not cache and _captured(graphed) == 1
  _assert_same_model(eager, graphed)
  assert int(graphed.optimizer.iterations) == 12      # the float steps do not tick


def test_a_device_tensor_learning_rate_changes_between_replays_without_a_recapture():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(34)
  batches = _batches(rng, [512] * 3)
  lr = torch.tensor(0.5, device="cuda")
  graphed = _quickstart(tfrs, lambda m: tfrs.optimizers.Adagrad(m.parameters(), learning_rate=lr))
  by_float = _quickstart(tfrs, lambda m: tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.5))
  hg = graphed.fit(batches, epochs=2)
  hf = by_float.fit(batches, epochs=2, graph=False)
  cache = graphed.__dict__["_fit_graphs"]
  assert _captured(graphed) == 1
  before = [_np(p).copy() for p in graphed.parameters()]
  lr.fill_(0.05)
  for group in by_float.optimizer.param_groups:
    group["learning_rate"] = float(np.float32(0.05))
  hg2 = graphed.fit(batches, epochs=1)
  hf2 = by_float.fit(batches, epochs=1, graph=False)
  assert graphed.__dict__["_fit_graphs"] is cache and _captured(graphed) == 1       # no re-capture
  assert hg == hf and hg2 == hf2
  for a, b, old in zip(graphed.parameters(), by_float.parameters(), before):
    np.testing.assert_array_equal(_np(a), _np(b))
    assert not np.array_equal(_np(a), old)
    np.testing.assert_array_equal(_np(graphed.optimizer.state[a]["accumulator"]),
                                  _np(by_float.optimizer.state[b]["accumulator"]))


def test_a_constant_float_learning_rate_launches_no_tick_and_keeps_its_state_dict(monkeypatch):
  import recommenders_amd as tfrs
  from recommenders_amd import _lib
  from recommenders_amd.experimental.optimizers import ClippyAdagrad
  lib = _lib.load()
  calls = []
  for entry in ("tfrs_lr_tick", "tfrs_adam_tick_scheduled"):
    real = getattr(lib, entry)
    monkeypatch.setattr(lib, entry, lambda *a, _real=real, _name=entry: (calls.append(_name), _real(*a))[1])
  expected = {"Adagrad": {"accumulator"}, "SGD": set(), "Adam": {"step", "alpha", "m", "v"},
              "Ftrl": {"accumulator", "linear"}, "ClippyAdagrad": {"accumulator"}}
  for name, keys in expected.items():
    cls, kwargs = _optimizer(name)
    table = _table(50, 8, torch.Generator().manual_seed(1))
    dense = torch.nn.Parameter(torch.randn(33, 7, device="cuda"))
    opt = cls([table, dense], learning_rate=0.1, **kwargs)
    for _ in range(2):
      table._tfrs_slices.append((torch.randint(0, 50, (40,), device="cuda"), torch.randn(40, 8, device="cuda")))
      dense.grad = torch.randn_like(dense)
      opt.step()
    assert {k for st in opt.state_dict()["state"].values() for k in st} == keys, name
    opt.close()
  assert calls == []
  # the wrapper does count: a scheduled optimizer ticks once per step
  p = torch.nn.Parameter(torch.randn(5, device="cuda"))
  opt = tfrs.optimizers.SGD([p], learning_rate=schedules.ExponentialDecay(0.1, 4, 0.5))
  p.grad = torch.randn_like(p)
  opt.step()
  assert calls == ["tfrs_lr_tick"]
