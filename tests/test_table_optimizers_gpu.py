"""``optimizers.SGD`` / ``Adam`` / ``Ftrl`` on the MI355X: ``tfrs_table_update_sparse`` on both routes,
``tfrs_table_update_dense_multi`` and ``tfrs_adam_tick`` against the float64 restatement on the kernels' own float32
state under the derived bounds of tests/table_optimizers_restatement.py (which tests/test_table_optimizers_host.py holds
the float32 restatement itself to), untouched rows bit for bit, run-to-run bit-reproducibility, models trained through
captured steps, and the ``state_dict`` round trip."""

import copy

import numpy as np
import pytest
import torch

from tests import clippy_restatement as crs
from tests import table_optimizers_restatement as rs

pytestmark = pytest.mark.gpu

NAMES = sorted(rs.RULES)


def _np(t):
  return t.detach().cpu().numpy()


def _bits(t):
  return _np(t).view(np.uint32) if t.dtype == torch.float32 else _np(t)


def _cls(kind):
  from recommenders_amd import optimizers
  return getattr(optimizers, kind)


def _table(values):
  p = torch.nn.Parameter(torch.as_tensor(np.asarray(values)).cuda())
  p._tfrs_embedding = True
  return p


def _report(name, used):
  print(f"{name}: fraction of each budget used: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(used.items())))


def _worst(worst, used):
  for k, v in used.items():
    worst[k] = max(worst.get(k, 0.0), v)


def _optimizer_on_table(name, table, slots):
  kind, hp = rs.RULES[name]
  p = _table(table)
  opt = _cls(kind)([p], **hp)
  for key, s in zip(rs.SLOTS[kind], slots):
    opt.state[p][key] = torch.as_tensor(s).cuda()
  return p, opt


def _slices_step(p, opt, ids, rows):
  p._tfrs_slices.append((torch.as_tensor(ids).cuda(), torch.as_tensor(rows).cuda()))
  opt.step()
  assert p.grad is None and p._tfrs_slices == []


def _state(p, opt, kind):
  return [p.detach()] + [opt.state[p][key] for key in rs.SLOTS[kind]]


# ---- 1. sparse, both routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("d", crs.SPARSE_DIMS)
def test_sparse_kernels_stay_inside_the_derived_bounds_both_routes(d, name):
  """A row-scan shape and a sorted-route shape at every d (d % 4 != 0: the scalar segments), int32 and int64 ids,
  duplicates -- on the sorted route a run that crosses several piece boundaries --, negative, out-of-range and INT_MAX
  ids, a touched row whose summed gradient is exactly zero; two consecutive steps, each compared from the kernels' own
  float32 state; untouched rows of the table and of every slot bit for bit."""
  from recommenders_amd.layers import embedding as emb
  kind, hp = rs.RULES[name]
  worst, moved = {}, 1.0
  piece = rs.piece_length(d)
  for case in rs.sparse_cases(d):
    vocab, n = case["vocab"], case["n"]
    rowscan = vocab == 3000
    assert emb._use_rowscan(vocab, n, d) == rowscan
    p, opt = _optimizer_on_table(name, case["table"], rs.start_slots(name, case["table"], case["acc"]))
    for t, (ids, rows) in enumerate(case["steps"], start=1):
      valid = ids[(ids >= 0) & (ids < vocab)]
      assert np.unique(valid).size < valid.size < ids.size
      if not rowscan:
        assert np.bincount(valid).max() > 3 * piece
      before = [s.clone() for s in _state(p, opt, kind)]
      _slices_step(p, opt, ids, rows)
      after = _state(p, opt, kind)
      uniq, g = rs.sum_duplicates(ids, rows, vocab, None if rowscan else piece)      # (the order this route sums in)
      if t == 1:
        assert (g == 0).all(axis=1).any()           # the touched row whose summed gradient is exactly zero
      rows_idx = torch.as_tensor(uniq).cuda()
      w0, s0 = _np(before[0][rows_idx]), [_np(s[rows_idx]) for s in before[1:]]
      alpha = None
      if kind == "Adam":
        alpha = rs.adam_alpha(hp, t)
        assert int(opt.iterations) == t
        worst["alpha"] = max(worst.get("alpha", 0.0), rs.check_alpha(float(opt.state[p]["alpha"]), hp, t))
      ref = rs.update(kind, w0, s0, g, hp, np.float64, alpha)
      got = [_np(s[rows_idx]) for s in after]
      label = f"{name} d {d} vocab {vocab} step {t}"
      compared = got[0].size
      assert compared >= 0.95 * uniq.size * d and compared == ref["w"].size
      _worst(worst, rs.check_step(kind, got[0], got[1:], w0, ref, g, label=label))
      moved = min(moved, rs.moved_fraction(kind, ref, g, w0))
      untouched = torch.ones((vocab,), dtype=torch.bool, device="cuda")
      untouched[rows_idx] = False
      for key, a, b in zip(("w",) + rs.SLOTS[kind], after, before):
        assert torch.equal(a[untouched].view(torch.int32), b[untouched].view(torch.int32)), f"{label}: untouched rows of {key}"
  _report(f"sparse {name} d {d}", worst)
  print(f"sparse {name} d {d}: moved by > 100 bounds on {moved:.4f} of the touched elements with a gradient")
  assert moved >= 0.95


# ---- 2. the summed gradient is the Adagrad path's -----------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 128])
def test_sgd_at_rate_one_on_a_zero_table_is_minus_the_scatter_add(d):
  from recommenders_amd.layers import embedding as emb
  from recommenders_amd.optimizers import SGD
  for case in rs.sparse_cases(d):
    vocab = case["vocab"]
    ids, rows = case["steps"][0]
    p = _table(np.zeros((vocab, d), np.float32))
    opt = SGD([p], learning_rate=1.0)
    _slices_step(p, opt, ids, rows)
    dense = emb.scatter_add_rows(torch.as_tensor(rows).cuda(), torch.as_tensor(ids).cuda(), vocab)
    assert bool((dense != 0).any())
    assert torch.equal(p.detach(), -dense), f"vocab {vocab} d {d}"


# ---- 3. dense -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_dense_kernel_stays_inside_the_derived_bounds(name):
  """40 tensors of awkward sizes (1, 7, a size that ends in the middle of a 16-byte piece and of a block, whole blocks;
  every third one a view 4 bytes into its storage: the scalar path) -- two calls of ``tfrs_table_update_dense_multi``
  per step -- two steps; every step is compared from the kernels' own float32 state."""
  kind, hp = rs.RULES[name]
  sizes, ws, all_grads = rs.dense_case(name)
  base = [torch.as_tensor(np.r_[w, np.float32(7.0)]).cuda() for w in ws]
  params = [torch.nn.Parameter(b.roll(1)[1:] if i % 3 == 2 else b[:-1].clone()) for i, b in enumerate(base)]
  assert any(p.data_ptr() % 16 for p in params) and len(params) == 40
  opt = _cls(kind)(params, **hp)
  worst = {}
  for t, grads in enumerate(all_grads, start=1):
    before = [[_np(p)] + ([_np(opt.state[p][k]) for k in rs.SLOTS[kind]] if t > 1 else rs.initial_slots(kind, hp, _np(p)))
              for p in params]
    for p, g in zip(params, grads):
      p.grad = torch.as_tensor(g).cuda()
    opt.step()
    alpha = None
    if kind == "Adam":
      alpha = rs.adam_alpha(hp, t)
      worst["alpha"] = max(worst.get("alpha", 0.0), rs.check_alpha(float(opt.state[params[0]]["alpha"]), hp, t))
    for i, (p, g, b) in enumerate(zip(params, grads, before)):
      ref = rs.update(kind, b[0], b[1:], g, hp, np.float64, alpha)
      _worst(worst, rs.check_step(kind, _np(p), [_np(opt.state[p][k]) for k in rs.SLOTS[kind]], b[0], ref, g,
                                  label=f"{name} tensor {i} (n={sizes[i]}) step {t}"))
  _report(f"dense {name}", worst)


# ---- 4. no ids, or none valid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sgd", "adam", "ftrl_reg"])
def test_a_lookup_without_valid_ids_writes_nothing_and_adam_still_counts(name):
  from recommenders_amd.layers import embedding as emb
  kind, hp = rs.RULES[name]
  rng = np.random.default_rng(5)
  for vocab in (100, 300_000):
    table = crs.weights(rng, (vocab, 32))
    p, opt = _optimizer_on_table(name, table, rs.start_slots(name, table, np.full_like(table, 0.1)))
    invalid = np.resize(np.array([-1, vocab, -7, 2 ** 40], np.int64), 4 if vocab == 100 else 300)
    assert emb._use_rowscan(vocab, invalid.size, 32) == (vocab == 100)         # both routes see ids of which none is valid
    for ids in (np.zeros((0,), np.int64), invalid):
      rows = crs.gradients(rng, (ids.size, 32), outliers=True) if ids.size else np.zeros((0, 32), np.float32)
      before = [s.clone() for s in _state(p, opt, kind)]
      _slices_step(p, opt, ids, rows)
      for a, b in zip(_state(p, opt, kind), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kind == "Adam":
      assert int(opt.iterations) == 2
      opt.step()              # no slices and no gradient at all
      assert int(opt.iterations) == 3


def test_adam_updates_a_looked_up_row_whose_summed_gradient_is_exactly_zero():
  """Lazy Adam still decays the moments of a row that was looked up with r + (-r), and moves it by its momentum; on
  both routes."""
  from recommenders_amd.layers import embedding as emb
  from recommenders_amd.optimizers import Adam
  rng = np.random.default_rng(6)
  for vocab in (100, 300_000):
    assert emb._use_rowscan(vocab, 300, 8) == (vocab == 100)
    table = crs.weights(rng, (vocab, 8))
    p = _table(table)
    opt = Adam([p], learning_rate=0.01)
    ids = rng.integers(0, vocab, size=300)
    ids[:2] = 17
    rows = crs.gradients(rng, (300, 8), outliers=False) + np.float32(1e-3)
    _slices_step(p, opt, ids, rows)
    m1, v1, w1 = (_np(x[17]) for x in (opt.state[p]["m"], opt.state[p]["v"], p))
    assert (m1 != 0).all()
    ids2 = np.where(ids == 17, 18, ids)
    ids2[:2] = 17
    rows2 = rows.copy()
    rows2[1] = -rows2[0]
    _slices_step(p, opt, ids2, rows2)
    ref = rs.update("Adam", w1, [m1, v1], np.zeros((8,), np.float32), rs.RULES["adam"][1] | dict(learning_rate=0.01),
                    np.float32, float(opt.state[p]["alpha"]))
    np.testing.assert_array_equal(_np(opt.state[p]["m"][17]), ref["slots"][0])
    np.testing.assert_array_equal(_np(opt.state[p]["v"][17]), ref["slots"][1])
    np.testing.assert_array_equal(_np(p[17]), ref["w"])
    assert (ref["w"] != w1).all() and (ref["slots"][0] != m1).all()


# ---- 5. bit reproducibility ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_steps_are_bit_reproducible(name):
  """The same step from the same state twice: both sparse routes (duplicate sums are sequential, long runs are cut at
  fixed positions) and dense tensors."""
  kind, hp = rs.RULES[name]
  cases = rs.sparse_cases(32)
  sparse = [cases[0], cases[2]]
  rng = np.random.default_rng(11)
  sizes = [130_001, 4096 * 16 + 3, 77]
  ws = [crs.weights(rng, (n,)) for n in sizes]
  gs = [crs.gradients(rng, (n,), outliers=True) for n in sizes]
  runs = []
  for _ in range(2):
    out = []
    for case in sparse:
      p, opt = _optimizer_on_table(name, case["table"], rs.start_slots(name, case["table"], case["acc"]))
      for ids, rows in case["steps"]:
        _slices_step(p, opt, ids, rows)
      out += [_bits(s) for s in _state(p, opt, kind)]
    params = [torch.nn.Parameter(torch.as_tensor(w).cuda()) for w in ws]
    opt = _cls(kind)(params, **hp)
    for p, g in zip(params, gs):
      p.grad = torch.as_tensor(g).cuda()
    opt.step()
    for p in params:
      out += [_bits(s) for s in _state(p, opt, kind)]
    runs.append(out)
  assert len(runs[0]) == len(runs[1]) >= 5
  for a, b in zip(*runs):
    assert np.array_equal(a, b)


# ---- 6. captured steps --------------------------------------------------------------------------------------------------
def _tower(tfrs):
  class Tower(tfrs.Model):
    """Two embedding tables (a row-scan sized one and one on the sorted route) feeding a small MLP."""

    def __init__(self):
      super().__init__()
      self.small = tfrs.layers.embedding.Embedding(3000, 32)
      self.big = tfrs.layers.embedding.Embedding(400_000, 32)
      self.mlp = tfrs.layers.blocks.MLP([64, 1])

    def compute_loss(self, inputs, training=False):
      x = torch.cat([self.small(inputs["a"]), self.big(inputs["b"])], dim=-1)
      return (self.mlp(x).squeeze(-1) - inputs["y"]).square().mean()

  torch.manual_seed(1234)
  model = Tower().cuda()
  example = {"a": torch.zeros(8, dtype=torch.int64, device="cuda"), "b": torch.zeros(8, dtype=torch.int64, device="cuda"),
             "y": torch.zeros(8, device="cuda")}
  with torch.no_grad():
    model.compute_loss(example)       # (builds the lazily created MLP kernels)
  return model


def _batches(seed, count=4):
  rng = np.random.default_rng(seed)
  return [{"a": torch.as_tensor(crs.zipf_ids(rng, 512, 3000)).cuda(), "b": torch.as_tensor(crs.zipf_ids(rng, 512, 400_000)).cuda(),
           "y": torch.as_tensor((rng.normal(size=(512,)) * 3).astype(np.float32)).cuda()} for _ in range(count)]


def _same_training_state(eager, graphed):
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_bits(a), _bits(b))
  compared = 0
  for pa, pb in zip(eager.parameters(), graphed.parameters()):
    sa, sb = eager.optimizer.state.get(pa, {}), graphed.optimizer.state.get(pb, {})
    assert set(sa) == set(sb)
    for key in sa:
      np.testing.assert_array_equal(_bits(sa[key]), _bits(sb[key]), err_msg=key)
      compared += 1
  return compared


def _build(kind):
  import recommenders_amd as tfrs
  from recommenders_amd.experimental.optimizers import CompositeOptimizer
  model = _tower(tfrs)
  tables = [model.small.embeddings, model.big.embeddings]
  dense = [p for p in model.parameters() if all(p is not t for t in tables)]
  assert len(dense) == 4
  if kind == "adam":
    model.compile(optimizer=tfrs.optimizers.Adam(model.parameters(), learning_rate=0.01))
  elif kind == "sgd":
    model.compile(optimizer=tfrs.optimizers.SGD(model.parameters(), learning_rate=0.05))
  else:
    ftrl = tfrs.optimizers.Ftrl(tables, learning_rate=0.05, l1_regularization_strength=1e-4, beta=0.1)
    adam = torch.optim.Adam(dense, lr=0.01, capturable=True)
    model.compile(optimizer=CompositeOptimizer([(ftrl, lambda: tables), (adam, lambda: dense)]))
  return model, tables


@pytest.mark.parametrize("kind", ["adam", "ftrl_composite", "sgd"])
def test_fit_through_captured_steps_walks_the_eager_trajectory_bit_for_bit(kind):
  """Four steps eagerly and four through ``fit(graph=True)`` from one seed: parameters, slots and Adam's counter are
  bitwise equal, and the counter is 4 -- not 4 plus the warm-up iteration of the capture, which a counter kept outside
  ``optimizer.state`` would show."""
  batches = _batches(31)
  (eager, _), (graphed, tables) = _build(kind), _build(kind)
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a), _np(b))
  start = [_np(t).copy() for t in tables]
  assert graphed._graph_steps_allowed(None, training=True) is True          # also the default of `fit`
  he = eager.fit(batches, epochs=1, graph=False)
  hg = graphed.fit(batches, epochs=1, graph=True)
  assert he == hg
  cache = graphed.__dict__["_fit_graphs"]
  assert sum(callable(v) for v in cache.values()) == 1 and "_errors" not in cache, cache
  assert not eager.__dict__.get("_fit_graphs")
  compared = _same_training_state(eager, graphed)
  assert compared >= (0 if kind == "sgd" else 12)
  if kind == "adam":
    assert int(graphed.optimizer.iterations) == 4 and int(eager.optimizer.iterations) == 4
  for t, s in zip(tables, start):
    assert t.grad is None and t._tfrs_sparse_grad
    assert not np.array_equal(_np(t), s)
  graphed.optimizer.close()
  assert not any(t._tfrs_sparse_grad for t in tables)


def test_adam_counter_is_rolled_back_when_a_step_is_captured_before_any_step():
  """``make_graphed_train_step`` on a fresh optimizer: the three warm-up iterations and the capture create the slots and
  advance the counter; ``reset_state_`` puts all of it back, so four replays are four eager steps."""
  batches = _batches(32)
  (eager, _), (graphed, _) = _build("adam"), _build("adam")
  step = graphed.make_graphed_train_step(batches[0], warmup=3)
  assert int(graphed.optimizer.iterations) == 0
  for batch in batches:
    step(batch)
    eager.train_step(batch)
  assert int(graphed.optimizer.iterations) == 4
  assert _same_training_state(eager, graphed) >= 14


# ---- 7. state_dict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "ftrl_reg"])
def test_state_dict_round_trip_continues_the_run_bit_for_bit(name):
  kind, hp = rs.RULES[name]
  rng = np.random.default_rng(41)
  table0, dense0 = crs.weights(rng, (5000, 16)), crs.weights(rng, (777,))
  steps = [(crs.zipf_ids(rng, 2048, 5000), crs.gradients(rng, (2048, 16), outliers=False), crs.gradients(rng, (777,), outliers=False))
           for _ in range(4)]

  def make(table, dense):
    p, q = _table(table), torch.nn.Parameter(torch.as_tensor(dense).cuda())
    return p, q, _cls(kind)([p, q], **hp)

  def run(p, q, opt, some):
    for ids, rows, g in some:
      q.grad = torch.as_tensor(g).cuda()
      _slices_step(p, opt, ids, rows)

  p, q, opt = make(table0, dense0)
  run(p, q, opt, steps[:2])
  saved = copy.deepcopy(opt.state_dict())
  p2, q2, fresh = make(_np(p), _np(q))
  fresh.load_state_dict(saved)
  run(p, q, opt, steps[2:])
  run(p2, q2, fresh, steps[2:])
  for a, b in ((p, p2), (q, q2)):
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert set(opt.state[a]) == set(fresh.state[b])
    for key in opt.state[a]:
      np.testing.assert_array_equal(_bits(opt.state[a][key]), _bits(fresh.state[b][key]), err_msg=key)
  if kind == "Adam":
    assert int(fresh.iterations) == 4 and fresh.state[p2]["step"].is_cuda


# ---- a configured front-end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "ftrl_reg", "sgd"])
def test_tpu_embedding_hands_its_slices_to_the_new_optimizers(name):
  """Two features on one table (a ragged one with a mean combiner and a plain one): one combined IndexedSlices per
  table, no dense ``[vocab, d]`` gradient, and the step is the restatement's on those slices."""
  from recommenders_amd.layers.embedding import FeatureConfig, RaggedIds, TableConfig, TPUEmbedding
  kind, hp = rs.RULES[name]
  rng = np.random.default_rng(12)
  vocab, d, nrows = 500, 16, 128
  table0 = crs.weights(rng, (vocab, d))
  tc = TableConfig(vocabulary_size=vocab, dim=d, initializer=lambda s: table0, combiner="mean", name="t")
  layer = TPUEmbedding({"a": FeatureConfig(table=tc), "b": FeatureConfig(table=tc)})
  opt = _cls(kind)(layer.parameters(), **hp)
  lengths = rng.integers(0, 5, size=nrows)
  splits = np.r_[0, np.cumsum(lengths)].astype(np.int64)
  ids_a, ids_b = rng.integers(0, vocab, size=int(splits[-1])), rng.integers(0, vocab, size=(nrows,))
  out = layer({"a": RaggedIds(torch.as_tensor(ids_a).cuda(), splits), "b": torch.as_tensor(ids_b).cuda()})
  ga, gb = (torch.as_tensor(crs.gradients(rng, (nrows, d), outliers=False)).cuda() for _ in range(2))
  opt.zero_grad()
  ((out["a"] * ga).sum() + (out["b"] * gb).sum()).backward()
  p = layer.embedding_tables[tc]
  assert p.grad is None and len(p._tfrs_slices) >= 1          # no dense [vocab, d] gradient was built
  ids_all = np.concatenate([_np(s[0]).reshape(-1) for s in p._tfrs_slices])
  rows_all = np.concatenate([_np(s[1]).reshape(-1, d) for s in p._tfrs_slices])
  opt.step()
  slots0 = rs.initial_slots(kind, hp, table0)
  alpha = rs.adam_alpha(hp, 1) if kind == "Adam" else None
  ref = rs.sparse_update(kind, table0, slots0, ids_all, rows_all, hp, np.float64, alpha)
  uniq = ref["uniq"]
  got_slots = [_np(opt.state[p][key])[uniq] for key in rs.SLOTS[kind]]
  _report(f"TPUEmbedding {name}", rs.check_step(kind, _np(p)[uniq], got_slots, table0[uniq], ref, ref["g"]))
  untouched = np.setdiff1d(np.arange(vocab), uniq)
  assert untouched.size and np.array_equal(_np(p)[untouched], table0[untouched])
