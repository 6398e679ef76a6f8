"""``ClippyAdagrad`` / ``CompositeOptimizer`` on the MI355X: the two-pass kernels ``tfrs_clippy_dense_multi`` and
``tfrs_clippy_sparse`` against the float64 restatement on the same float32 inputs under the derived bounds of
tests/clippy_restatement.py (which tests/test_clippy_host.py holds the float32 restatement itself to), the clipping
guarantee element by element, run-to-run bit-reproducibility, and a model trained through captured steps."""

import numpy as np
import pytest
import torch

from tests import clippy_restatement as rs

pytestmark = pytest.mark.gpu


def _np(t):
  return t.detach().cpu().numpy()


def _table(values):
  p = torch.nn.Parameter(torch.as_tensor(values).cuda())
  p._tfrs_embedding = True
  return p


def _report(name, used):
  print(f"{name}: fraction of each budget used: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(used.items())))


def _worst(worst, used):
  for k, v in used.items():
    worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_clippy_dense_kernels_stay_inside_the_derived_bounds(mode):
  """40 tensors of awkward sizes (1, 7, a size that ends in the middle of a 16-byte piece and of a block, whole blocks;
  every third one a view 4 bytes into its storage: the scalar path) -- two calls of ``tfrs_clippy_dense_multi`` -- two
  steps; every step is compared from the kernels' own float32 state.  Half of the tensors carry outlier gradients."""
  from recommenders_amd.experimental.optimizers import ClippyAdagrad
  hp, sizes, ws, all_grads = rs.dense_case(mode)
  base = [torch.as_tensor(np.r_[w, np.float32(7.0)]).cuda() for w in ws]
  # (every third parameter is a view that starts 4 bytes into its storage: not 16-byte aligned)
  params = [torch.nn.Parameter(b.roll(1)[1:] if i % 3 == 2 else b[:-1].clone()) for i, b in enumerate(base)]
  assert any(p.data_ptr() % 16 for p in params) and len(params) == 40
  opt = ClippyAdagrad(params, **hp)
  factors, worst = [], {}
  for step in range(2):
    before = [(_np(p), _np(opt.state[p]["accumulator"]) if p in opt.state else np.full((p.numel(),), 0.1, np.float32))
              for p in params]
    grads = all_grads[step]
    for p, g in zip(params, grads):
      p.grad = torch.as_tensor(g).cuda()
    opt.step()
    for i, (p, g, (w0, a0)) in enumerate(zip(params, grads, before)):
      ref = rs.update(w0, a0, g, hp, np.float64)
      _worst(worst, rs.check_step(_np(p), _np(opt.state[p]["accumulator"]), float(opt.clipping_factors[i]), w0, ref, g, hp,
                                  label=f"mode {mode} tensor {i} (n={sizes[i]}) step {step}"))
      factors.append(float(opt.clipping_factors[i]))
  _report(f"dense mode {mode}", worst)
  assert any(f < 1.0 for f in factors) and any(f == 1.0 for f in factors)
  assert all(0.0 < f <= 1.0 for f in factors)


def _run_sparse(table, acc, ids, rows, hp):
  """One ``ClippyAdagrad`` step on the slices; returns (table', acc', factor) as numpy."""
  from recommenders_amd.experimental.optimizers import ClippyAdagrad
  p = _table(table)
  opt = ClippyAdagrad([p], **hp)
  opt.state[p]["accumulator"] = torch.as_tensor(acc).cuda()
  p._tfrs_slices.append((torch.as_tensor(ids).cuda(), torch.as_tensor(rows).cuda()))
  opt.step()
  torch.cuda.synchronize()
  assert p.grad is None
  return _np(p), _np(opt.state[p]["accumulator"]), float(opt.clipping_factors[0])


def _check_sparse(table, acc, ids, rows, hp, label):
  got_w, got_acc, got_f = _run_sparse(table, acc, ids, rows, hp)
  ref = rs.sparse_update(table, acc, ids, rows, hp, np.float64)
  uniq = ref["uniq"]
  used = rs.check_step(got_w[uniq], got_acc[uniq], got_f, table[uniq], ref, ref["g"], hp, label=label)
  untouched = np.ones((table.shape[0],), bool)
  untouched[uniq] = False
  assert np.array_equal(got_w[untouched].view(np.uint32), table[untouched].view(np.uint32)), f"{label}: untouched table rows"
  assert np.array_equal(got_acc[untouched].view(np.uint32), acc[untouched].view(np.uint32)), f"{label}: untouched accumulator rows"
  zero_rows = uniq[(ref["g"] == 0).all(axis=1)]
  assert np.array_equal(got_w[zero_rows], table[zero_rows])         # delta == 0: factor-neutral, weight unchanged
  return got_f, used, (got_w, got_acc)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d", rs.SPARSE_DIMS)
def test_clippy_sparse_kernels_stay_inside_the_derived_bounds_both_routes(d, mode):
  """A row-scan shape (small vocab x n) and a sorted-route shape for every d the sparse Adagrad accepts (d % 4 != 0:
  the scalar segments), int32 and int64 ids, duplicates, negative / out-of-range ids, a touched row with an exactly
  zero summed gradient; untouched rows bitwise unchanged; with and without outlier gradients."""
  from recommenders_amd.layers import embedding as emb
  rng = rs.sparse_rng(mode, d)
  hp = rs.hyper(mode)
  factors, worst = [], {}
  for vocab, n, outliers, id_dtype in rs.SPARSE_SHAPES:
    assert emb._use_rowscan(vocab, n, d) == (vocab == 3000)
    table, acc, ids, rows = rs.sparse_case(rng, vocab, n, d, outliers, id_dtype)
    valid = ids[(ids >= 0) & (ids < vocab)]
    assert np.unique(valid).size < valid.size < ids.size
    f, used, _ = _check_sparse(table, acc, ids, rows, hp, f"mode {mode} d {d} vocab {vocab} outliers {outliers}")
    factors.append(f)
    _worst(worst, used)
  _report(f"sparse mode {mode} d {d}", worst)
  assert any(f < 1.0 for f in factors) and any(f == 1.0 for f in factors)


def test_clippy_sparse_sorted_route_on_a_large_table_with_zipf_ids():
  """2 M x 128 table, 1 M Zipf ids (the hottest id occurs ~10^5 times: one long run summed in occurrence order)."""
  rng = np.random.default_rng(77)
  vocab, n, d = 2_000_000, 1_000_000, 128
  hp = rs.hyper(1)
  table, acc = rs.weights(rng, (vocab, d)), np.full((vocab, d), 0.1, np.float32)
  ids = rs.zipf_ids(rng, n, vocab)
  ids[::97] = -1
  ids[5::101] = vocab + 3
  rows = rs.gradients(rng, (n, d), outliers=True)
  f, used, _ = _check_sparse(table, acc, ids, rows, hp, "2M x 128, 1M Zipf ids")
  _report("sparse 2M x 128", used)
  assert np.bincount(ids[(ids >= 0) & (ids < vocab)]).max() > 10_000
  assert 0.0 < f < 1.0


def test_clippy_sparse_without_ids_writes_nothing_and_reports_factor_one():
  rng = np.random.default_rng(5)
  for vocab in (100, 300_000):
    table, acc = rs.weights(rng, (vocab, 32)), np.full((vocab, 32), 0.1, np.float32)
    for ids in (np.zeros((0,), np.int64), np.array([-1, vocab, -7], np.int64)):      # none, and none that is valid
      rows = rs.gradients(rng, (ids.size, 32), outliers=True) if ids.size else np.zeros((0, 32), np.float32)
      w, a, f = _run_sparse(table, acc, ids, rows, rs.hyper(0))
      assert f == 1.0
      assert np.array_equal(w.view(np.uint32), table.view(np.uint32)) and np.array_equal(a.view(np.uint32), acc.view(np.uint32))


def test_clippy_steps_are_bit_reproducible():
  """Two runs from the same state give the same bits (the factor is a min: order-independent; duplicate sums are
  sequential): dense tensors and both sparse routes."""
  from recommenders_amd.experimental.optimizers import ClippyAdagrad
  rng = np.random.default_rng(11)
  hp = rs.hyper(1)
  sparse = [rs.sparse_case(rng, 3000, 4096, 32, True), rs.sparse_case(rng, 300_000, 50_000, 128, True)]
  sizes = [130_001, 4096 * 16 + 3, 77]
  ws = [rs.weights(rng, (n,)) for n in sizes]
  gs = [rs.gradients(rng, (n,), outliers=True) for n in sizes]
  runs = []
  for _ in range(2):
    out = [_run_sparse(*case, hp) for case in sparse]
    params = [torch.nn.Parameter(torch.as_tensor(w).cuda()) for w in ws]
    opt = ClippyAdagrad(params, **hp)
    for p, g in zip(params, gs):
      p.grad = torch.as_tensor(g).cuda()
    opt.step()
    out += [(_np(p), _np(opt.state[p]["accumulator"]), float(f)) for p, f in zip(params, opt.clipping_factors)]
    runs.append(out)
  for (w1, a1, f1), (w2, a2, f2) in zip(*runs):
    assert f1 == f2 and f1 < 1.0
    assert np.array_equal(w1.view(np.uint32), w2.view(np.uint32)) and np.array_equal(a1.view(np.uint32), a2.view(np.uint32))


def test_clippy_c_abi_rejects_bad_arguments():
  import ctypes
  from recommenders_amd import _lib
  lib = _lib.load()
  t = torch.ones(8, device="cuda")
  vp, i64a = ctypes.c_void_p * 1, ctypes.c_int64 * 1
  args = (vp(t.data_ptr()), vp(t.data_ptr()), vp(t.data_ptr()), i64a(8), _lib.ptr(t))
  with pytest.raises(ValueError, match="mode"):
    _lib.check(lib.tfrs_clippy_dense_multi(1, *args, 0.1, 1e-7, 0.1, 0.0, 1e-7, 3, _lib.current_stream()))
  with pytest.raises(ValueError, match="1..32"):
    _lib.check(lib.tfrs_clippy_dense_multi(33, *args, 0.1, 1e-7, 0.1, 0.0, 1e-7, 0, _lib.current_stream()))
  with pytest.raises(ValueError, match="non-negative"):
    _lib.check(lib.tfrs_clippy_dense_multi(1, *args, 0.1, 1e-7, -0.1, 0.0, 1e-7, 0, _lib.current_stream()))
  with pytest.raises(ValueError, match="d=300"):
    _lib.check(lib.tfrs_clippy_sparse(_lib.ptr(t), _lib.ptr(t), 1, 1, 300, 10, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 0.1, 1e-7,
                                      0.1, 0.0, 1e-7, 0, 1, None, 0, _lib.current_stream()))
  assert lib.tfrs_clippy_sparse_workspace_bytes(1000, 0) == lib.tfrs_embedding_scatter_add_workspace_bytes(1000)
  with pytest.raises(RuntimeError, match="workspace too small"):
    _lib.check(lib.tfrs_clippy_sparse(_lib.ptr(t), _lib.ptr(t), 1, 1, 8, 10, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 0.1, 1e-7,
                                      0.1, 0.0, 1e-7, 0, 0, _lib.ptr(t), 8, _lib.current_stream()))
  torch.cuda.synchronize()


# ---- model level --------------------------------------------------------------------------------------------------------
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


def test_model_trains_tables_with_clippy_and_dense_weights_with_adagrad_through_captured_steps():
  """``CompositeOptimizer([(ClippyAdagrad(tables)), (Adagrad(dense))])``: ``fit`` replays captured steps by default and
  walks the eager trajectory bit for bit -- parameters, accumulators, exported clipping factors -- and no dense
  ``[vocab, d]`` gradient is ever built for the tables."""
  import recommenders_amd as tfrs
  from recommenders_amd.experimental.optimizers import ClippyAdagrad, CompositeOptimizer
  rng = np.random.default_rng(21)
  batches = []
  for _ in range(6):
    b = rs.zipf_ids(rng, 512, 400_000)
    batches.append({"a": torch.as_tensor(rs.zipf_ids(rng, 512, 3000)).cuda(), "b": torch.as_tensor(b).cuda(),
                    "y": torch.as_tensor((rng.normal(size=(512,)) * 30).astype(np.float32)).cuda()})

  def build():
    model = _tower(tfrs)
    tables = [model.small.embeddings, model.big.embeddings]
    dense = [p for p in model.parameters() if all(p is not t for t in tables)]
    assert len(dense) == 4
    clippy = ClippyAdagrad(tables, learning_rate=0.5, export_clipping_factors=True, clip_accumulator_update=True)
    model.compile(optimizer=CompositeOptimizer([(clippy, lambda: tables), (tfrs.optimizers.Adagrad(dense, learning_rate=0.05), lambda: dense)]))
    return model, clippy, tables

  (eager, clippy_e, tables_e), (graphed, clippy_g, tables_g) = build(), build()
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a), _np(b))
  start = [_np(t).copy() for t in tables_g]
  assert graphed._graph_steps_allowed(None, training=True) is True
  factors_e, factors_g = [], []
  for epoch in range(3):
    he = eager.fit(batches, epochs=1, graph=False)
    hg = graphed.fit(batches, epochs=1)
    assert he == hg
    factors_e.append([float(f) for f in clippy_e.clipping_factors])
    factors_g.append([float(f) for f in clippy_g.clipping_factors])
  cache = graphed.__dict__["_fit_graphs"]
  assert sum(callable(v) for v in cache.values()) == 1 and "_errors" not in cache, cache
  assert not eager.__dict__.get("_fit_graphs")
  assert factors_e == factors_g
  assert any(f < 1.0 for fs in factors_g for f in fs), factors_g       # the clipping was exercised
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a).view(np.uint32), _np(b).view(np.uint32))
  for pa, pb in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(eager.optimizer.state[pa]["accumulator"]).view(np.uint32),
                                  _np(graphed.optimizer.state[pb]["accumulator"]).view(np.uint32))
  for t, s in zip(tables_g, start):
    assert t.grad is None and t._tfrs_sparse_grad
    assert not np.array_equal(_np(t), s)
  graphed.optimizer.close()
  assert not any(t._tfrs_sparse_grad for t in tables_g)


def test_composite_with_a_capturable_torch_member_replays_the_eager_trajectory():
  """``CompositeOptimizer([ClippyAdagrad(tables), Adam(dense, capturable=True)])``: Adam keeps ``step`` / ``exp_avg`` /
  ``exp_avg_sq`` and creates them lazily.  (a) ``fit`` captures a shape at its second sighting, when every member has
  state: the warm-up is rolled back member by member and the replayed trajectory is the eager one bit for bit, Adam's
  state included.  (b) a capture before any step: Adam's state cannot be put back, so NOTHING is -- the warm-up
  iterations stay applied as ordinary steps for every member (the documented outcome for lazily created torch.optim
  state), never for Adam alone."""
  import recommenders_amd as tfrs
  from recommenders_amd.experimental.optimizers import ClippyAdagrad, CompositeOptimizer
  rng = np.random.default_rng(22)
  batches = []
  for _ in range(5):
    batches.append({"a": torch.as_tensor(rs.zipf_ids(rng, 512, 3000)).cuda(),
                    "b": torch.as_tensor(rs.zipf_ids(rng, 512, 400_000)).cuda(),
                    "y": torch.as_tensor((rng.normal(size=(512,)) * 30).astype(np.float32)).cuda()})

  def build():
    model = _tower(tfrs)
    tables = [model.small.embeddings, model.big.embeddings]
    dense = [p for p in model.parameters() if all(p is not t for t in tables)]
    clippy = ClippyAdagrad(tables, learning_rate=0.5, export_clipping_factors=True)
    adam = torch.optim.Adam(dense, lr=0.01, capturable=True)
    model.compile(optimizer=CompositeOptimizer([(clippy, lambda: tables), (adam, lambda: dense)]))
    return model, adam, dense

  def same_state(eager, graphed):
    for a, b in zip(eager[0].parameters(), graphed[0].parameters()):
      np.testing.assert_array_equal(_np(a).view(np.uint32), _np(b).view(np.uint32))
    for pa, pb in zip(eager[0].parameters(), graphed[0].parameters()):
      sa, sb = eager[0].optimizer.state[pa], graphed[0].optimizer.state[pb]
      assert set(sa) == set(sb) and sa
      for key in sa:
        np.testing.assert_array_equal(_np(sa[key]), _np(sb[key]), err_msg=key)

  # (a) fit
  eager, graphed = build(), build()
  assert graphed[0]._graph_steps_allowed(None, training=True) is True
  for _ in range(2):
    assert eager[0].fit(batches, epochs=1, graph=False) == graphed[0].fit(batches, epochs=1)
  cache = graphed[0].__dict__["_fit_graphs"]
  assert sum(callable(v) for v in cache.values()) == 1 and "_errors" not in cache, cache
  same_state(eager, graphed)
  assert float(graphed[1].state[graphed[2][0]]["step"]) == 10.0
  # (b) capture first: the three warm-up iterations stay applied, for every member alike
  eager, graphed = build(), build()
  step = graphed[0].make_graphed_train_step(batches[0], warmup=3)
  for _ in range(3):
    eager[0].train_step(batches[0])
  same_state(eager, graphed)
  for batch in batches[1:]:
    step(batch)
    eager[0].train_step(batch)
  same_state(eager, graphed)
