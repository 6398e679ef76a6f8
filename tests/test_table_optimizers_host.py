"""``optimizers.SGD`` / ``Adam`` / ``Ftrl`` without a GPU: constructor validation, the torch-op route (CPU tensors,
float64) against the float64 restatement of tests/table_optimizers_restatement.py, that restatement against independent
implementations (``torch.optim.SparseAdam``, ``torch.optim.SGD``, the legacy Adagrad step for Ftrl), the float32
restatement held to the derived bounds -- the bounds the kernels are then held to in tests/test_table_optimizers_gpu.py --
the argument checks of the C entries, and the cross-compiled kernels (no scratch, no spills)."""

import copy
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import recommenders_amd as tfrs
from recommenders_amd import _lib
from recommenders_amd.optimizers import Adam, Ftrl, SGD
from tests import clippy_restatement as crs
from tests import table_optimizers_restatement as rs

CLASSES = {"SGD": SGD, "Adam": Adam, "Ftrl": Ftrl}


def _table(values, dtype=torch.float32):
  """A parameter that takes ``(ids, rows)`` slices like an ``Embedding`` table."""
  p = torch.nn.Parameter(torch.as_tensor(np.asarray(values), dtype=dtype))
  p._tfrs_embedding = True
  return p


# ---- constructors -----------------------------------------------------------------------------------------------------
def test_constructor_validation_and_config():
  w = lambda: [torch.nn.Parameter(torch.ones(3))]
  with pytest.raises(NotImplementedError):
    SGD(w(), momentum=0.9)
  with pytest.raises(NotImplementedError):
    SGD(w(), nesterov=True)
  for kwargs in (dict(l1_regularization_strength=-1.0), dict(l2_regularization_strength=-1.0),
                 dict(l2_shrinkage_regularization_strength=-1.0), dict(learning_rate_power=0.5),
                 dict(initial_accumulator_value=-0.1)):
    with pytest.raises(ValueError):
      Ftrl(w(), **kwargs)
  with pytest.raises(NotImplementedError, match="-0.5 or 0"):
    Ftrl(w(), learning_rate_power=-0.3)
  with pytest.raises(ValueError):
    Adam(w(), beta_1=1.0)
  with pytest.raises(TypeError):
    Adam(w(), amsgrad=True)
  with pytest.raises(TypeError):
    Adam(w(), weight_decay=0.1)
  assert SGD(w()).get_config() == dict(learning_rate=0.01)
  assert Adam(w()).get_config() == dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
  assert Ftrl(w()).get_config() == dict(
      learning_rate=0.001, learning_rate_power=-0.5, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
      l2_regularization_strength=0.0, l2_shrinkage_regularization_strength=0.0, beta=0.0)
  for cls in (SGD, Adam, Ftrl):
    opt = cls(w(), learning_rate=0.25)
    again = cls.from_config(w(), opt.get_config())
    assert again.get_config() == opt.get_config() and isinstance(opt, tfrs.optimizers.SliceOwningOptimizer)


def test_tables_hand_slices_to_the_latest_optimizer_and_close_releases_them():
  table = _table(np.ones((4, 2), np.float32))
  first = Adam([table])
  assert table._tfrs_sparse_grad and first._owns(table)
  second = Ftrl([table])
  first.close()
  assert table._tfrs_sparse_grad and second._owns(table)
  second.close()
  assert not table._tfrs_sparse_grad


# ---- the torch-op route of the optimizers against the float64 restatement ---------------------------------------------
@pytest.mark.parametrize("name", sorted(rs.RULES))
def test_torch_route_equals_the_float64_restatement_on_slices_and_dense(name):
  """CPU float64 parameters: a table with duplicate, negative and out-of-range ids and a dense tensor, three steps; rows
  that were not looked up are not written (lazy Adam, row-sparse Ftrl)."""
  kind, hp = rs.RULES[name]
  rng = np.random.default_rng(4)
  table0, dense0 = crs.weights(rng, (9, 5)).astype(np.float64), crs.weights(rng, (17,)).astype(np.float64)
  table, dense = _table(table0, torch.float64), torch.nn.Parameter(torch.as_tensor(dense0))
  opt = CLASSES[kind]([table, dense], **hp)
  want_t, want_d = table0.copy(), dense0.copy()
  slots_t, slots_d = rs.initial_slots(kind, hp, want_t), rs.initial_slots(kind, hp, want_d)
  ids = np.array([[4, 4, -1], [7, 9, 4], [0, 12, 7]])
  for t in (1, 2, 3):
    rows, g = crs.gradients(rng, (3, 3, 5), outliers=True), crs.gradients(rng, (17,), outliers=False).astype(np.float64)
    table._tfrs_slices.append((torch.as_tensor(ids), torch.as_tensor(rows)))
    dense.grad = torch.as_tensor(g)
    opt.step()
    alpha = np.float32(rs.adam_alpha(hp, t)) if kind == "Adam" else None       # (the optimizer keeps alpha in float32)
    ref = rs.sparse_update(kind, want_t, slots_t, ids, rows, hp, np.float64, alpha)
    np.testing.assert_array_equal(ref["uniq"], [0, 4, 7])
    want_t[ref["uniq"]] = ref["w"]
    for s, new in zip(slots_t, ref["slots"]):
      s[ref["uniq"]] = new
    refd = rs.update(kind, want_d, slots_d, g, hp, np.float64, alpha)
    want_d, slots_d = refd["w"], refd["slots"]
    np.testing.assert_allclose(table.detach().numpy(), want_t, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(dense.detach().numpy(), want_d, rtol=1e-12, atol=1e-300)
    for key, s_t, s_d in zip(rs.SLOTS[kind], slots_t, slots_d):
      np.testing.assert_allclose(opt.state[table][key].numpy(), s_t, rtol=1e-12, atol=1e-300)
      np.testing.assert_allclose(opt.state[dense][key].numpy(), s_d, rtol=1e-12, atol=1e-300)
    assert table.grad is None and table._tfrs_slices == []
  untouched = [1, 2, 3, 5, 6, 8]
  np.testing.assert_array_equal(table.detach().numpy()[untouched], table0[untouched])
  for key, init in zip(rs.SLOTS[kind], rs.initial_slots(kind, hp, table0)):
    np.testing.assert_array_equal(opt.state[table][key].numpy()[untouched], init[untouched])
  if kind == "Adam":
    assert int(opt.iterations) == 3 and opt.state[table]["step"].dtype == torch.int64


def test_adam_counter_advances_without_gradients_and_reset_and_state_dict_round_trip():
  rng = np.random.default_rng(9)
  w0 = crs.weights(rng, (6, 3))
  grads = [crs.gradients(rng, (6, 3), outliers=False) for _ in range(4)]

  def run(opt, p, steps):
    for g in steps:
      p.grad = torch.as_tensor(g)
      opt.step()

  p = torch.nn.Parameter(torch.as_tensor(w0.copy()))
  opt = Adam([p], learning_rate=0.01)
  opt.step()                       # no gradient anywhere: the counter still advances
  assert int(opt.iterations) == 1 and torch.equal(p.detach(), torch.as_tensor(w0))
  storage = {k: v.data_ptr() for k, v in opt.state[p].items()}
  opt.reset_state_()
  assert int(opt.iterations) == 0 and {k: v.data_ptr() for k, v in opt.state[p].items()} == storage
  assert all(float(opt.state[p][k].abs().max()) == 0.0 for k in ("m", "v"))
  run(opt, p, grads[:2])
  saved = copy.deepcopy(opt.state_dict())
  q = torch.nn.Parameter(p.detach().clone())
  fresh = Adam([q], learning_rate=0.5)
  fresh.load_state_dict(saved)
  assert int(fresh.iterations) == 2 and fresh.state[q]["step"].dtype == torch.int64
  assert fresh.param_groups[0]["learning_rate"] == 0.01
  run(opt, p, grads[2:])
  run(fresh, q, grads[2:])
  assert torch.equal(p.detach(), q.detach()) and int(fresh.iterations) == 4
  for key in ("m", "v", "alpha"):
    assert torch.equal(opt.state[p][key], fresh.state[q][key])
  ftrl = Ftrl([p], initial_accumulator_value=0.3)
  run(ftrl, p, grads[:1])
  ftrl.reset_state_()
  assert torch.all(ftrl.state[p]["accumulator"] == 0.3) and torch.all(ftrl.state[p]["linear"] == 0.0)


# ---- the float64 restatement against independent implementations ------------------------------------------------------
def _exact_rows(rng, shape):
  """Multiples of 2^-10 below 1/2: float32 sums of a few duplicates are exact, so the order of a sum is immaterial."""
  return (rng.integers(-511, 512, size=shape) / 1024.0).astype(np.float32)


def test_adam_restatement_equals_torch_sparse_adam():
  """Five steps, vocab 50, dim 8, 20 ids per step with duplicates: lazy Adam is ``torch.optim.SparseAdam``."""
  rng = np.random.default_rng(0)
  kind, hp = rs.RULES["adam"]
  w = crs.weights(rng, (50, 8)).astype(np.float64)
  p = torch.nn.Parameter(torch.as_tensor(w.copy()))
  opt = torch.optim.SparseAdam([p], lr=hp["learning_rate"], betas=(hp["beta_1"], hp["beta_2"]), eps=hp["epsilon"])
  slots = rs.initial_slots(kind, hp, w)
  worst = 0.0
  for t in range(1, 6):
    ids = rng.integers(0, 50, size=20)
    ids[:2] = ids[2]
    rows = _exact_rows(rng, (20, 8))
    assert np.unique(ids).size < ids.size
    p.grad = torch.sparse_coo_tensor(torch.as_tensor(ids)[None], torch.as_tensor(rows, dtype=torch.float64), (50, 8))
    opt.step()
    ref = rs.sparse_update(kind, w, slots, ids, rows, hp, np.float64, rs.adam_alpha(hp, t))
    w[ref["uniq"]] = ref["w"]
    for s, new in zip(slots, ref["slots"]):
      s[ref["uniq"]] = new
    worst = max(worst, float(np.abs(p.detach().numpy() - w).max()))
  print(f"restatement vs SparseAdam: largest difference {worst:.3g}")
  assert worst <= 1e-12


def test_sgd_restatement_equals_torch_sgd():
  rng = np.random.default_rng(1)
  kind, hp = rs.RULES["sgd"]
  w = crs.weights(rng, (50, 8)).astype(np.float64)
  p = torch.nn.Parameter(torch.as_tensor(w.copy()))
  opt = torch.optim.SGD([p], lr=hp["learning_rate"])
  for _ in range(5):
    ids = rng.integers(0, 50, size=20)
    ids[:2] = ids[2]
    rows = _exact_rows(rng, (20, 8))
    p.grad = torch.sparse_coo_tensor(torch.as_tensor(ids)[None], torch.as_tensor(rows, dtype=torch.float64), (50, 8)).to_dense()
    opt.step()
    ref = rs.sparse_update(kind, w, [], ids, rows, hp, np.float64)
    w[ref["uniq"]] = ref["w"]
    assert float(np.abs(p.detach().numpy() - w).max()) <= 1e-12


def test_ftrl_without_regularisers_from_a_consistent_state_is_the_legacy_adagrad_step(lr=0.05):
  """l1 = l2 = shrink = beta = 0 and lin = -w sqrt(n) / lr: one Ftrl step is w - lr g / sqrt(n')."""
  rng = np.random.default_rng(2)
  w = crs.weights(rng, (40, 8)).astype(np.float64)
  n = rng.uniform(0.025, 0.225, size=w.shape)
  g = rng.normal(size=w.shape) * 0.1
  hp = dict(learning_rate=lr)
  lin = -w * np.sqrt(n) / lr
  out = rs.update("Ftrl", w, [n, lin], g, hp, np.float64)
  want = w - lr * g / np.sqrt(n + g * g)
  np.testing.assert_allclose(out["w"], want, rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(out["slots"][0], n + g * g, rtol=1e-15)


def test_ftrl_l1_gives_exact_zeros():
  rng = np.random.default_rng(3)
  hp = dict(learning_rate=0.1, l1_regularization_strength=0.05)
  w = crs.weights(rng, (500,))
  n, lin = np.full_like(w, 0.1), np.zeros_like(w)
  g = (rng.normal(size=w.shape) * 0.05).astype(np.float32)
  for dtype in (np.float32, np.float64):
    out = rs.update("Ftrl", w, [n, lin], g, hp, dtype)
    small = np.abs(out["slots"][1]) <= dtype(0.05)
    assert 50 < small.sum() < 450
    assert (out["w"][small] == 0.0).all() and (out["w"][~small] != 0.0).all()
  p = torch.nn.Parameter(torch.as_tensor(w.copy()))
  opt = Ftrl([p], **hp)
  p.grad = torch.as_tensor(g)
  opt.step()
  ref = rs.update("Ftrl", w, [n, lin], g, hp, np.float32)
  np.testing.assert_array_equal(p.detach().numpy() == 0.0, ref["w"] == 0.0)


# ---- the float32 restatement inside the derived bounds ----------------------------------------------------------------
def _worst(worst, used):
  for k, v in used.items():
    worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("d", crs.SPARSE_DIMS)
def test_float32_restatement_stays_inside_the_bounds_on_the_sparse_cases(d):
  """Every rule on the cases the GPU test runs, two consecutive steps from the float32 state; and the condition that
  makes the band check bite: the float64 step moves ``w`` by more than 100 x its bound on >= 95 % of the touched elements
  with a non-zero gradient."""
  for name in sorted(rs.RULES):
    kind, hp = rs.RULES[name]
    worst, moved = {}, 1.0
    for case in rs.sparse_cases(d):
      w = case["table"].copy()
      slots = [s.copy() for s in rs.start_slots(name, case["table"], case["acc"])]
      for t, (ids, rows) in enumerate(case["steps"], start=1):
        piece = None if case["vocab"] == 3000 else rs.piece_length(d)          # (as the GPU test: the route's own order)
        uniq, g = rs.sum_duplicates(ids, rows, case["vocab"], piece)
        w0, s0 = w[uniq], [s[uniq] for s in slots]
        alpha = rs.adam_alpha(hp, t) if kind == "Adam" else None
        ref = rs.update(kind, w0, s0, g, hp, np.float64, alpha)
        got = rs.update(kind, w0, s0, g, hp, np.float32, alpha)
        assert got["w"].dtype == np.float32
        _worst(worst, rs.check_step(kind, got["w"], got["slots"], w0, ref, g, label=f"{name} d {d} step {t}"))
        moved = min(moved, rs.moved_fraction(kind, ref, g, w0))
        w[uniq] = got["w"]             # the next step starts from the float32 state
        for s, new in zip(slots, got["slots"]):
          s[uniq] = new
    print(f"{name} d {d}: fraction of each budget used: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) +
          f"; moved by > 100 bounds: {moved:.4f}")
    assert moved >= 0.95, (name, moved)


@pytest.mark.parametrize("name", sorted(rs.RULES))
def test_float32_restatement_stays_inside_the_bounds_on_the_dense_sizes(name):
  kind, hp = rs.RULES[name]
  sizes, ws, all_grads = rs.dense_case(name)
  worst = {}
  for i, w in enumerate(ws):
    slots = rs.initial_slots(kind, hp, w)
    for t, grads in enumerate(all_grads, start=1):
      alpha = rs.adam_alpha(hp, t) if kind == "Adam" else None
      ref = rs.update(kind, w, slots, grads[i], hp, np.float64, alpha)
      got = rs.update(kind, w, slots, grads[i], hp, np.float32, alpha)
      _worst(worst, rs.check_step(kind, got["w"], got["slots"], w, ref, grads[i], label=f"{name} tensor {i} step {t}"))
      w, slots = got["w"], got["slots"]
  print(f"dense {name}: fraction of each budget used: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_alpha_bound_holds_for_the_float32_rounding():
  hp = rs.RULES["adam"][1]
  for t in (1, 2, 3, 10, 1000, 10 ** 6, 10 ** 9):
    rs.check_alpha(np.float32(rs.adam_alpha(hp, t)), hp, t)


# ---- the C entries ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  return _lib.load()


def test_c_entries_reject_bad_arguments_before_any_device_call(lib):
  """NULL device pointers throughout: a check that ran after a launch could not return these codes on a machine
  without a GPU."""
  h = lambda *v: (ctypes.c_float * 8)(*v)
  sparse = lambda rule, hyper, **kw: lib.tfrs_table_update_sparse(
      rule, hyper, kw.get("alpha"), None, None, 1, kw.get("n", 4), kw.get("d", 8), kw.get("vocab", 10), None, None, None,
      kw.get("rowscan", 0), None, 0, None)
  for call, text in [
      (lambda: sparse(3, h(0.1)), "rule must be"),
      (lambda: sparse(0, None), "NULL hyper"),
      (lambda: sparse(1, h(0.1, 0.001, 1e-7)), "tfrs_adam_tick"),
      (lambda: sparse(2, h(0.0, 0, 0, 0, -0.5)), "learning rate must be positive"),
      (lambda: sparse(2, h(0.1, -1.0, 0, 0, -0.5)), "non-negative"),
      (lambda: sparse(2, h(0.1, 0, 0, 0, -0.3)), "-0.5 or 0"),
      (lambda: sparse(0, h(0.1), d=0), "bad shape"),
      (lambda: sparse(0, h(0.1), vocab=1 << 33), "32 bits"),
      (lambda: sparse(0, h(0.1)), "NULL pointer"),
      (lambda: sparse(0, h(0.1), d=300, rowscan=1), "NULL pointer"),
      (lambda: lib.tfrs_table_update_dense_multi(0, h(0.1), None, 0, None, None, None, None, None, None), "1..32"),
      (lambda: lib.tfrs_table_update_dense_multi(0, h(0.1), None, 33, None, None, None, None, None, None), "1..32"),
      (lambda: lib.tfrs_table_update_dense_multi(0, h(0.1), None, 1, None, None, None, None, None, None), "NULL argument array"),
      (lambda: lib.tfrs_table_update_dense_multi(7, h(0.1), None, 1, None, None, None, None, None, None), "rule must be"),
      (lambda: lib.tfrs_adam_tick(None, None, 0.001, 0.9, 0.999, 1, None), "NULL pointer"),
  ]:
    rc = call()
    assert rc == _lib.TFRS_EINVAL and text in _lib.last_error(), (rc, text, _lib.last_error())
  one = (ctypes.c_void_p * 1)(16)
  assert lib.tfrs_table_update_dense_multi(1, h(0.1, 0.001, 1e-7), ctypes.c_void_p(16), 1, one, None, None, one,
                                           (ctypes.c_int64 * 1)(4), None) == _lib.TFRS_EINVAL       # Adam without slots
  step, alpha = ctypes.c_void_p(16), ctypes.c_void_p(32)
  assert lib.tfrs_adam_tick(step, alpha, 0.001, 1.0, 0.999, 1, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_adam_tick(step, alpha, 0.001, 0.9, 0.999, 2, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_table_update_workspace_bytes(1000, 0) == lib.tfrs_embedding_scatter_add_workspace_bytes(1000)
  assert lib.tfrs_table_update_workspace_bytes(1000, 1) == 256


def test_new_source_is_built():
  from recommenders_amd.csrc import build as csrc_build
  assert "table_update.hip" in csrc_build.SOURCES


@pytest.mark.parametrize("source,expected", [("sparse_update.hip", 20), ("table_update.hip", 5)])
def test_table_update_kernels_use_no_scratch_and_do_not_spill(source, expected):
  """From the code object metadata of the cross-compiled source: every ``table_update_*`` kernel and the tick."""
  from recommenders_amd.csrc import build as csrc_build
  src = os.path.join(os.path.dirname(csrc_build.__file__), source)
  out = os.path.join(tempfile.mkdtemp(prefix="tfrs_table_update_"), source + ".s")
  subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17",
                  *csrc_build.EXTRA_FLAGS.get(source, []), "-S", "--cuda-device-only", "-o", out, src],
                 check=True, capture_output=True, cwd=os.path.dirname(src))
  with open(out) as f:
    asm = f.read()
  found = 0
  for block in asm.split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", block).group(1)
    if "table_update" not in name and "adam_tick" not in name:
      continue
    found += 1
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  # sparse_update.hip: 4 rules (Ftrl twice: sqrt and power 0) x (2 row-scan id types + 3 sorted forms);
  # table_update.hip: 4 dense kernels and the tick
  assert found == expected
