"""``optimizers.RowWiseAdagrad`` on the MI355X: ``tfrs_rowwise_adagrad_sparse`` on both routes and
``tfrs_rowwise_adagrad_dense`` against the float64 restatement on the kernels' own float32 state under the derived
bounds of tests/rowwise_adagrad_restatement.py (which tests/test_rowwise_adagrad_host.py holds the float32 restatement
itself to), untouched rows bit for bit, run-to-run bit-reproducibility, a model trained through captured steps, the
``TPUEmbedding`` hand-over and the argument checks of the C entries."""

import numpy as np
import pytest
import torch

from tests import clippy_restatement as crs
from tests import rowwise_adagrad_restatement as rw
from tests import table_optimizers_restatement as rs

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 32, 64, 128, 200, 520]


def _np(t):
  return t.detach().cpu().numpy()


def _bits(t):
  return _np(t).view(np.uint32) if t.dtype == torch.float32 else _np(t)


def _opt(params, **kw):
  from recommenders_amd.optimizers import RowWiseAdagrad
  return RowWiseAdagrad(params, **kw)


def _table(values):
  p = torch.nn.Parameter(torch.as_tensor(np.asarray(values)).cuda())
  p._tfrs_embedding = True
  return p


def _on_table(table, acc, **hp):
  p = _table(table)
  opt = _opt([p], **hp)
  opt.state[p]["accumulator"] = torch.as_tensor(np.asarray(acc)).cuda()
  return p, opt


def _slices_step(p, opt, ids, rows):
  p._tfrs_slices.append((torch.as_tensor(ids).cuda(), torch.as_tensor(rows).cuda()))
  opt.step()
  assert p.grad is None and p._tfrs_slices == []


def _same_bits(a, b):
  return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. sparse, both routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("d", DIMS)
def test_sparse_kernels_stay_inside_the_derived_bounds_both_routes(d, legacy):
  """The four sparse cases at every d: vocab 3000 takes the row scan (up to its limit d = 256; d = 520 goes through the
  sorted route there too), vocab 300 000 the sorted route with a run that crosses several piece boundaries; d % 4 != 0
  is the scalar path, d = 200 a lane group with idle lanes, d = 520 more than one chunk per lane; int32 and int64 ids,
  duplicates, negative, out-of-range and INT_MAX ids, a touched row whose summed gradient is exactly zero; two
  consecutive steps, each compared from the kernels' own float32 state; untouched rows bit for bit."""
  from recommenders_amd.layers import embedding as emb
  hp = rw.hyper(legacy)
  worst, moved = {}, 1.0
  piece = rs.piece_length(d)
  for case in rs.sparse_cases(d):
    vocab, n = case["vocab"], case["n"]
    rowscan = vocab == 3000 and d <= 256
    assert emb._use_rowscan(vocab, n, d) == rowscan
    p, opt = _on_table(case["table"], rw.row_accumulator(case), **hp)
    for t, (ids, rows) in enumerate(case["steps"], start=1):
      valid = ids[(ids >= 0) & (ids < vocab)]
      assert np.unique(valid).size < valid.size < ids.size
      if vocab == 300_000:     # (the longest run is about 1900 positions: 3 pieces up to d = 256, one cut at d = 520)
        assert np.bincount(valid).max() > (3 if d <= 256 else 1) * piece
      acc = opt.state[p]["accumulator"]
      assert acc.shape == (vocab,) and acc.dtype == torch.float32
      w_before, a_before = p.detach().clone(), acc.clone()
      _slices_step(p, opt, ids, rows)
      assert opt.state[p]["accumulator"] is acc
      uniq, g = rs.sum_duplicates(ids, rows, vocab, None if rowscan else piece)      # (the order this route sums in)
      zero = (g == 0).all(axis=1)
      if t == 1:
        assert zero.any()           # the touched row whose summed gradient is exactly zero
      idx = torch.as_tensor(uniq).cuda()
      w0, a0 = _np(w_before[idx]), _np(a_before[idx])
      ref = rw.update(w0, a0, g, hp, np.float64)
      label = f"d {d} vocab {vocab} legacy {legacy} step {t}"
      used = rw.check_step(_np(p.detach()[idx]), _np(acc[idx]), ref, g, label=label)
      for k, v in used.items():
        worst[k] = max(worst.get(k, 0.0), v)
      moved = min(moved, rw.moved_fraction(ref, g, w0))
      untouched = torch.ones((vocab,), dtype=torch.bool, device="cuda")
      untouched[idx] = False
      assert _same_bits(p.detach()[untouched], w_before[untouched]), f"{label}: untouched rows of w"
      assert _same_bits(acc[untouched], a_before[untouched]), f"{label}: untouched rows of the accumulator"
      zidx = idx[torch.as_tensor(zero).cuda()]
      assert _same_bits(p.detach()[zidx], w_before[zidx]) and _same_bits(acc[zidx], a_before[zidx]), f"{label}: zero-sum row"
  print(f"sparse d {d} legacy {legacy}: fraction of each budget used {worst}; moved {moved:.4f}")
  assert moved >= 0.95


# ---- 2. dense -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (1000, 64), (4099, 128), (257, 200), (33, 520)])
def test_dense_kernel_stays_inside_the_derived_bounds(shape, legacy):
  """Every row of a 2-D parameter; every fifth gradient row is all zero and keeps its bits; once 16-byte aligned (the
  float4 path where d % 4 == 0) and once as a view 4 bytes into its storage (the scalar path); two steps."""
  hp = rw.hyper(legacy)
  rows, d = shape
  rng = np.random.default_rng(900 + rows)
  w0 = crs.weights(rng, shape)
  grads = [crs.gradients(rng, shape, outliers=True) for _ in range(2)]
  for g in grads:
    g[::5] = 0
  for misaligned in (False, True):
    if misaligned:
      base = torch.zeros((rows * d + 1,), device="cuda")
      base[1:] = torch.as_tensor(w0).cuda().reshape(-1)
      p = torch.nn.Parameter(base[1:].view(rows, d))
      assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    else:
      p = torch.nn.Parameter(torch.as_tensor(w0).cuda())
    opt = _opt([p], **hp)
    w_prev, a_prev = w0, np.full((rows,), 0.1, np.float32)
    for t, g in enumerate(grads, start=1):
      p.grad = torch.as_tensor(g).cuda()
      opt.step()
      acc = opt.state[p]["accumulator"]
      assert acc.shape == (rows,) and acc.dtype == torch.float32
      ref = rw.update(w_prev, a_prev, g, hp, np.float64)
      used = rw.check_step(_np(p), _np(acc), ref, g, label=f"dense {shape} misaligned {misaligned} step {t}")
      assert np.array_equal(_np(p)[::5].view(np.uint32), w_prev[::5].view(np.uint32))
      assert np.array_equal(_np(acc)[::5].view(np.uint32), a_prev[::5].view(np.uint32))
      print(f"dense {shape} legacy {legacy} misaligned {misaligned} step {t}: {used}")
      w_prev, a_prev = _np(p).copy(), _np(acc).copy()


# ---- 3. no ids, or none valid -------------------------------------------------------------------------------------------
def test_a_lookup_without_valid_ids_writes_nothing_on_either_route():
  from recommenders_amd.layers import embedding as emb
  rng = np.random.default_rng(5)
  for vocab in (100, 300_000):
    table = crs.weights(rng, (vocab, 32))
    p, opt = _on_table(table, np.full((vocab,), 0.1, np.float32), **rw.hyper())
    invalid = np.resize(np.array([-1, vocab, -7, 2 ** 40], np.int64), 4 if vocab == 100 else 300)
    assert emb._use_rowscan(vocab, invalid.size, 32) == (vocab == 100)         # both routes see ids of which none is valid
    for ids in (np.zeros((0,), np.int64), invalid):
      rows = crs.gradients(rng, (ids.size, 32), outliers=True) if ids.size else np.zeros((0, 32), np.float32)
      w_before, a_before = p.detach().clone(), opt.state[p]["accumulator"].clone()
      _slices_step(p, opt, ids, rows)
      assert _same_bits(p.detach(), w_before) and _same_bits(opt.state[p]["accumulator"], a_before)


# ---- 4. bit reproducibility ---------------------------------------------------------------------------------------------
def test_steps_are_bit_reproducible():
  """The same steps from the same state twice: both sparse routes (the duplicate sums and the order of the d additions
  are fixed) and a dense parameter."""
  cases = rs.sparse_cases(32)
  rng = np.random.default_rng(11)
  w, g = crs.weights(rng, (4099, 72)), crs.gradients(rng, (4099, 72), outliers=True)
  runs = []
  for _ in range(2):
    out = []
    for case in (cases[0], cases[2]):
      p, opt = _on_table(case["table"], rw.row_accumulator(case), **rw.hyper())
      for ids, rows in case["steps"]:
        _slices_step(p, opt, ids, rows)
      out += [_bits(p), _bits(opt.state[p]["accumulator"])]
    q = torch.nn.Parameter(torch.as_tensor(w).cuda())
    opt = _opt([q], **rw.hyper())
    q.grad = torch.as_tensor(g).cuda()
    opt.step()
    out += [_bits(q), _bits(opt.state[q]["accumulator"])]
    runs.append(out)
  assert len(runs[0]) == len(runs[1]) == 6
  for a, b in zip(*runs):
    assert np.array_equal(a, b)
  assert not np.array_equal(runs[0][0], _bits(torch.as_tensor(cases[0]["table"])))


# ---- 5. captured steps --------------------------------------------------------------------------------------------------
def _two_tower(tfrs):
  class TwoTower(tfrs.Model):
    """A user tower on a row-scan sized table and an item tower on a table of the sorted route, a dense layer each."""

    def __init__(self):
      super().__init__()
      self.users = tfrs.layers.embedding.Embedding(3000, 32)
      self.items = tfrs.layers.embedding.Embedding(400_000, 32)
      self.user_tower = tfrs.layers.blocks.MLP([16])
      self.item_tower = tfrs.layers.blocks.MLP([16])

    def compute_loss(self, inputs, training=False):
      u = self.user_tower(self.users(inputs["user"]))
      v = self.item_tower(self.items(inputs["item"]))
      return ((u * v).sum(dim=-1) - inputs["y"]).square().mean()

  torch.manual_seed(4321)
  model = TwoTower().cuda()
  example = {"user": torch.zeros(8, dtype=torch.int64, device="cuda"), "item": torch.zeros(8, dtype=torch.int64, device="cuda"),
             "y": torch.zeros(8, device="cuda")}
  with torch.no_grad():
    model.compute_loss(example)       # (builds the lazily created MLP kernels)
  return model


def _batches(seed, count=4):
  rng = np.random.default_rng(seed)
  return [{"user": torch.as_tensor(crs.zipf_ids(rng, 512, 3000)).cuda(),
           "item": torch.as_tensor(crs.zipf_ids(rng, 512, 400_000)).cuda(),
           "y": torch.as_tensor((rng.normal(size=(512,)) * 3).astype(np.float32)).cuda()} for _ in range(count)]


def _build(scheduled):
  import recommenders_amd as tfrs
  from recommenders_amd.experimental.optimizers import CompositeOptimizer
  model = _two_tower(tfrs)
  tables = [model.users.embeddings, model.items.embeddings]
  dense = [p for p in model.parameters() if all(p is not t for t in tables)]
  assert len(dense) == 4
  lr = tfrs.schedules.ExponentialDecay(0.05, 2, 0.5) if scheduled else 0.05
  rowwise = tfrs.optimizers.RowWiseAdagrad(tables, learning_rate=lr)
  adagrad = tfrs.optimizers.Adagrad(dense, learning_rate=0.05)
  model.compile(optimizer=CompositeOptimizer([(rowwise, lambda: tables), (adagrad, lambda: dense)]))
  return model, tables, rowwise


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


@pytest.mark.parametrize("scheduled", [False, True])
def test_fit_through_captured_steps_walks_the_eager_trajectory_bit_for_bit(scheduled):
  """Four steps eagerly and four through ``fit(graph=True)`` from one seed, tables under ``RowWiseAdagrad`` and dense
  layers under ``Adagrad`` in one ``CompositeOptimizer``: parameters, accumulators and (with a schedule) the counter are
  bitwise equal, and the counter is 4 -- not 4 plus the warm-up iteration of the capture."""
  batches = _batches(33)
  (eager, _, ropt_e), (graphed, tables, ropt_g) = _build(scheduled), _build(scheduled)
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
  assert _same_training_state(eager, graphed) >= 6
  for t in tables:
    acc = ropt_g.state[t]["accumulator"]
    assert acc.shape == (t.shape[0],) and acc.dtype == torch.float32 and bool((acc != 0.1).any())
  if scheduled:
    assert int(ropt_g.iterations) == 4 and int(ropt_e.iterations) == 4
  else:
    assert ropt_g.iterations is None
  for t, s in zip(tables, start):
    assert t.grad is None and t._tfrs_sparse_grad
    assert not np.array_equal(_np(t), s)
  graphed.optimizer.close()
  assert not any(t._tfrs_sparse_grad for t in tables)


# ---- 6. a configured front-end ------------------------------------------------------------------------------------------
def test_tpu_embedding_hands_its_slices_to_rowwise_adagrad():
  """Two features on one table (a ragged one with a mean combiner and a plain one): one combined IndexedSlices per
  table, no dense ``[vocab, d]`` gradient, and the step is the restatement's on those slices."""
  from recommenders_amd.layers.embedding import FeatureConfig, RaggedIds, TableConfig, TPUEmbedding
  hp = rw.hyper()
  rng = np.random.default_rng(12)
  vocab, d, nrows = 500, 16, 128
  table0 = crs.weights(rng, (vocab, d))
  tc = TableConfig(vocabulary_size=vocab, dim=d, initializer=lambda s: table0, combiner="mean", name="t")
  layer = TPUEmbedding({"a": FeatureConfig(table=tc), "b": FeatureConfig(table=tc)})
  opt = _opt(layer.parameters(), **hp)
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
  uniq, g = rs.sum_duplicates(ids_all, rows_all, vocab)
  ref = rw.update(table0[uniq], np.full((uniq.size,), 0.1, np.float32), g, hp, np.float64)
  acc = opt.state[p]["accumulator"]
  assert acc.shape == (vocab,)
  print("TPUEmbedding:", rw.check_step(_np(p)[uniq], _np(acc)[uniq], ref, g))
  untouched = np.setdiff1d(np.arange(vocab), uniq)
  assert untouched.size and np.array_equal(_np(p)[untouched], table0[untouched])
  assert np.array_equal(_np(acc)[untouched], np.full((untouched.size,), 0.1, np.float32))


# ---- 7. the C entries ---------------------------------------------------------------------------------------------------
def test_c_entries_reject_bad_arguments_without_touching_the_device():
  """NULL table, d < 1, a bad mode, a too-small workspace, ...: the error code and the message, and the memory the valid
  pointers of the call name is untouched."""
  from recommenders_amd import _lib
  lib = _lib.load()
  for call, code, text in rw.c_entry_argument_cases(lib):
    rc = call()
    assert rc == code and text in _lib.last_error(), (rc, code, text, _lib.last_error())
  table = torch.ones((10, 8), device="cuda")
  acc = torch.full((10,), 0.1, device="cuda")
  g, ids = torch.ones((4, 8), device="cuda"), torch.arange(4, device="cuda")
  ws = torch.empty((lib.tfrs_table_update_workspace_bytes(4, 0),), dtype=torch.uint8, device="cuda")
  sparse = lambda table_ptr, d, mode, ws_bytes: lib.tfrs_rowwise_adagrad_sparse(
      _lib.ptr(g), _lib.ptr(ids), 1, 4, d, 10, table_ptr, _lib.ptr(acc), 0.1, None, 1e-7, mode, 0, _lib.ptr(ws), ws_bytes,
      _lib.current_stream())
  assert sparse(None, 8, 1, ws.numel()) == _lib.TFRS_EINVAL and "NULL pointer" in _lib.last_error()
  assert sparse(_lib.ptr(table), 0, 1, ws.numel()) == _lib.TFRS_EINVAL and "bad shape" in _lib.last_error()
  assert sparse(_lib.ptr(table), 8, 5, ws.numel()) == _lib.TFRS_EINVAL and "mode must be" in _lib.last_error()
  assert sparse(_lib.ptr(table), 8, 1, ws.numel() - 1) == _lib.TFRS_ENOMEM and "workspace too small" in _lib.last_error()
  torch.cuda.synchronize()
  assert bool((table == 1).all()) and bool((acc == 0.1).all())
  assert sparse(_lib.ptr(table), 8, 1, ws.numel()) == _lib.TFRS_OK          # (the same call with nothing wrong)
  torch.cuda.synchronize()
  assert bool((table[:4] != 1).all()) and bool((table[4:] == 1).all()) and bool((acc[:4] != 0.1).all())
