"""``optimizers.RowWiseAdagrad`` without a GPU: the float32 restatement and the torch-op route on CPU tensors against the
float64 restatement under the derived bounds of tests/rowwise_adagrad_restatement.py, untouched rows bit for bit, the
accumulator's shape, the constructor's errors, config and ``state_dict`` round trips, schedules, and the argument checks
of the two C entries."""

import copy
import ctypes

import numpy as np
import pytest
import torch

from recommenders_amd import _lib
from tests import clippy_restatement as crs
from tests import rowwise_adagrad_restatement as rw
from tests import table_optimizers_restatement as rs

DIMS = crs.SPARSE_DIMS + [520]


def _opt(params, **kw):
  from recommenders_amd.optimizers import RowWiseAdagrad
  return RowWiseAdagrad(params, **kw)


def _table(values):
  p = torch.nn.Parameter(torch.as_tensor(np.array(values)))
  p._tfrs_embedding = True
  return p


def _bits(x):
  x = x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  return x.view(np.uint32) if x.dtype == np.float32 else x


# ---- 1. the float32 restatement is inside the bounds ------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_float32_restatement_stays_inside_the_derived_bounds(d):
  """Every sparse case at every d, both steps (the second from the float32 result of the first), both denominators, a
  sequential and a pairwise-tree float32 sum; and every band bites: >= 0.95 of the elements with a gradient move by
  more than 100 bounds."""
  worst, moved = {}, 1.0
  for case in rs.sparse_cases(d):
    vocab = case["vocab"]
    sums = [rs.sum_duplicates(ids, rows, vocab) for ids, rows in case["steps"]]
    assert (sums[0][1] == 0).all(axis=1).any()
    touched = np.union1d(sums[0][0], sums[1][0])
    for legacy in (False, True):
      hp = rw.hyper(legacy)
      for order in ("sequential", "pairwise"):
        # (the touched rows only: rows `touched[k]` of the table live at k)
        table, acc = case["table"][touched], rw.row_accumulator(case)[touched]
        for t, (ids, g) in enumerate(sums, start=1):
          uniq = np.searchsorted(touched, ids)
          w0, a0 = table[uniq], acc[uniq]
          ref = rw.update(w0, a0, g, hp, np.float64)
          got = rw.update(w0, a0, g, hp, np.float32, order)
          used = rw.check_step(got["w"], got["acc"], ref, g, label=f"d {d} vocab {vocab} legacy {legacy} {order} step {t}")
          for k, v in used.items():
            worst[k] = max(worst.get(k, 0.0), v)
          moved = min(moved, rw.moved_fraction(ref, g, w0))
          table[uniq], acc[uniq] = got["w"], got["acc"]
  print(f"restatement d {d}: fraction of each budget used {worst}; moved {moved:.4f}")
  assert moved >= 0.95


def test_each_denominator_fails_the_other_ones_check():
  """With ``epsilon = 2^-10`` the two denominators differ by far more than a bound: the check can tell them apart."""
  case = rs.sparse_cases(32)[0]
  ids, rows = case["steps"][0]
  uniq, g = rs.sum_duplicates(ids, rows, case["vocab"])
  w0, a0 = case["table"][uniq], rw.row_accumulator(case)[uniq]
  for legacy in (False, True):
    mine, other = rw.hyper(legacy, epsilon=2.0 ** -10), rw.hyper(not legacy, epsilon=2.0 ** -10)
    ref = rw.update(w0, a0, g, mine, np.float64)
    got = rw.update(w0, a0, g, mine, np.float32)
    rw.check_step(got["w"], got["acc"], ref, g)
    wrong = rw.update(w0, a0, g, other, np.float32)
    with pytest.raises(AssertionError, match="of the bound"):
      rw.check_step(wrong["w"], wrong["acc"], ref, g)


# ---- 2. the torch-op route on CPU tensors -----------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("d", [3, 64, 200])
def test_torch_route_on_cpu_slices_stays_inside_the_bounds(d, legacy):
  """Sparse slices with duplicates, negative, out-of-range and INT_MAX ids and a touched row whose summed gradient is
  exactly zero; two steps; untouched rows of the table and of the accumulator bit for bit."""
  hp = rw.hyper(legacy)
  moved = 1.0
  for case in rs.sparse_cases(d)[:2]:
    vocab = case["vocab"]
    p = _table(case["table"])
    opt = _opt([p], **hp)
    opt.state[p]["accumulator"] = torch.as_tensor(rw.row_accumulator(case).copy())
    for t, (ids, rows) in enumerate(case["steps"], start=1):
      valid = ids[(ids >= 0) & (ids < vocab)]
      assert np.unique(valid).size < valid.size < ids.size
      w_before, a_before = p.detach().numpy().copy(), opt.state[p]["accumulator"].numpy().copy()
      p._tfrs_slices.append((torch.as_tensor(ids), torch.as_tensor(rows)))
      opt.step()
      assert p.grad is None and p._tfrs_slices == []
      acc = opt.state[p]["accumulator"]
      assert acc.shape == (vocab,) and acc.dtype == torch.float32
      uniq, g = rs.sum_duplicates(ids, rows, vocab)
      zero = (g == 0).all(axis=1)
      if t == 1:
        assert zero.any()
      ref = rw.update(w_before[uniq], a_before[uniq], g, hp, np.float64)
      w_after, a_after = p.detach().numpy(), acc.numpy()
      rw.check_step(w_after[uniq], a_after[uniq], ref, g, label=f"cpu d {d} vocab {vocab} step {t}")
      moved = min(moved, rw.moved_fraction(ref, g, w_before[uniq]))
      untouched = np.setdiff1d(np.arange(vocab), uniq)
      assert untouched.size
      assert np.array_equal(_bits(w_after[untouched]), _bits(w_before[untouched]))
      assert np.array_equal(_bits(a_after[untouched]), _bits(a_before[untouched]))
      assert np.array_equal(_bits(w_after[uniq[zero]]), _bits(w_before[uniq[zero]]))
      assert np.array_equal(_bits(a_after[uniq[zero]]), _bits(a_before[uniq[zero]]))
  assert moved >= 0.95


@pytest.mark.parametrize("legacy", [False, True])
def test_torch_route_on_a_dense_cpu_gradient_stays_inside_the_bounds(legacy):
  hp = rw.hyper(legacy)
  rng = np.random.default_rng(77)
  for rows, d in ((1, 1), (7, 3), (257, 200)):
    w0 = crs.weights(rng, (rows, d))
    g = crs.gradients(rng, (rows, d), outliers=True)
    g[::5] = 0
    p = torch.nn.Parameter(torch.as_tensor(w0.copy()))
    opt = _opt([p], **hp)
    p.grad = torch.as_tensor(g)
    opt.step()
    acc = opt.state[p]["accumulator"]
    assert acc.shape == (rows,) and acc.dtype == torch.float32
    ref = rw.update(w0, np.full((rows,), 0.1, np.float32), g, hp, np.float64)
    rw.check_step(p.detach().numpy(), acc.numpy(), ref, g, label=f"cpu dense {rows}x{d}")
    assert np.array_equal(_bits(p.detach().numpy()[::5]), _bits(w0[::5]))          # all-zero gradient rows
    assert np.array_equal(_bits(acc.numpy()[::5]), _bits(np.full_like(acc.numpy()[::5], 0.1)))


# ---- 3. the constructor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5,), (2, 3, 4)])
def test_a_parameter_that_is_not_two_dimensional_is_refused(shape):
  table = _table(np.zeros((4, 2), np.float32))
  with pytest.raises(ValueError, match="CompositeOptimizer"):
    _opt([table, torch.nn.Parameter(torch.zeros(shape))])
  assert not getattr(table, "_tfrs_sparse_grad", False)        # the refused optimizer released the table
  with pytest.raises(ValueError, match="non-negative"):
    _opt([table], initial_accumulator_value=-1.0)


def test_it_is_exported_beside_adagrad_and_is_a_slice_owning_optimizer():
  import recommenders_amd as tfrs
  from recommenders_amd import optimizers
  assert tfrs.optimizers.RowWiseAdagrad is optimizers.RowWiseAdagrad
  assert issubclass(optimizers.RowWiseAdagrad, optimizers.SliceOwningOptimizer)
  p = _table(np.zeros((4, 2), np.float32))
  opt = _opt([p])
  assert opt.get_config() == dict(learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, legacy=False)
  assert p._tfrs_sparse_grad and opt.iterations is None
  opt.close()
  assert not p._tfrs_sparse_grad


# ---- 4. config and state_dict -----------------------------------------------------------------------------------------
def _steps(rng, vocab, d, count):
  return [(crs.zipf_ids(rng, 512, vocab), crs.gradients(rng, (512, d), outliers=False),
           crs.gradients(rng, (9, d), outliers=False)) for _ in range(count)]


def _run(p, q, opt, steps):
  for ids, rows, g in steps:
    q.grad = torch.as_tensor(g)
    p._tfrs_slices.append((torch.as_tensor(ids), torch.as_tensor(rows)))
    opt.step()


@pytest.mark.parametrize("scheduled", [False, True])
def test_config_and_state_dict_round_trip_continue_the_run_bit_for_bit(scheduled):
  from recommenders_amd import schedules
  from recommenders_amd.optimizers import RowWiseAdagrad
  rng = np.random.default_rng(43)
  vocab, d = 700, 16
  table0, dense0 = crs.weights(rng, (vocab, d)), crs.weights(rng, (9, d))
  steps = _steps(rng, vocab, d, 4)
  lr = schedules.ExponentialDecay(0.5, 2, 0.5) if scheduled else 0.5
  p, q = _table(table0), torch.nn.Parameter(torch.as_tensor(dense0.copy()))
  opt = RowWiseAdagrad([p, q], learning_rate=lr, initial_accumulator_value=0.2, epsilon=1e-6, legacy=True)
  _run(p, q, opt, steps[:2])
  saved = copy.deepcopy(opt.state_dict())
  p2, q2 = _table(p.detach().numpy()), torch.nn.Parameter(q.detach().clone())
  fresh = RowWiseAdagrad.from_config([p2, q2], opt.get_config())
  assert fresh.get_config() == opt.get_config()
  fresh.load_state_dict(saved)
  for a, b in ((p, p2), (q, q2)):
    acc = fresh.state[b]["accumulator"]
    assert acc.shape == (a.shape[0],) and acc.dtype == torch.float32
  _run(p, q, opt, steps[2:])
  _run(p2, q2, fresh, steps[2:])
  for a, b in ((p, p2), (q, q2)):
    assert np.array_equal(_bits(a), _bits(b))
    assert set(opt.state[a]) == set(fresh.state[b])
    for key in opt.state[a]:
      assert np.array_equal(_bits(opt.state[a][key]), _bits(fresh.state[b][key])), key
  assert not np.array_equal(p.detach().numpy(), table0)
  if scheduled:
    assert int(fresh.iterations) == 4 and fresh.iterations.dtype == torch.int64
  else:
    assert fresh.iterations is None
  opt.reset_state_()
  assert bool((opt.state[p]["accumulator"] == 0.2).all()) and opt.state[p]["accumulator"].shape == (vocab,)
  if scheduled:
    assert int(opt.iterations) == 0


# ---- 5. schedules -----------------------------------------------------------------------------------------------------
def test_a_schedule_advances_iterations_and_sets_the_rate_of_every_step():
  """Step t runs at ``float(np.float32(schedule(t)))``: the float64 restatement at that rate holds the result."""
  from recommenders_amd import schedules
  schedule = schedules.ExponentialDecay(256.0, 1, 0.25)
  case = rs.sparse_cases(32)[1]
  vocab = case["vocab"]
  p = _table(case["table"])
  opt = _opt([p], learning_rate=schedule)
  opt.state[p]["accumulator"] = torch.as_tensor(rw.row_accumulator(case).copy())
  assert int(opt.iterations) == 0
  for t, (ids, rows) in enumerate(case["steps"]):
    w_before, a_before = p.detach().numpy().copy(), opt.state[p]["accumulator"].numpy().copy()
    p._tfrs_slices.append((torch.as_tensor(ids), torch.as_tensor(rows)))
    opt.step()
    assert int(opt.iterations) == t + 1
    uniq, g = rs.sum_duplicates(ids, rows, vocab)
    rate = float(np.float32(schedule(t)))
    assert rate == 256.0 * 0.25 ** t
    ref = rw.update(w_before[uniq], a_before[uniq], g, rw.hyper(learning_rate=rate), np.float64)
    rw.check_step(p.detach().numpy()[uniq], opt.state[p]["accumulator"].numpy()[uniq], ref, g, label=f"step {t}")
    if t == 1:      # (the band tells the rates of the two steps apart)
      other = rw.update(w_before[uniq], a_before[uniq], g, rw.hyper(learning_rate=256.0), np.float64)
      with pytest.raises(AssertionError, match="of the bound"):
        rw.check_step(p.detach().numpy()[uniq], opt.state[p]["accumulator"].numpy()[uniq], other, g)


def test_a_composite_optimizer_takes_it_as_a_member():
  from recommenders_amd.experimental.optimizers import CompositeOptimizer
  from recommenders_amd.optimizers import Adagrad
  rng = np.random.default_rng(5)
  p, bias = _table(crs.weights(rng, (50, 4))), torch.nn.Parameter(torch.zeros(4))
  before = p.detach().clone()
  opt = CompositeOptimizer([(_opt([p], learning_rate=0.5), lambda: [p]), (Adagrad([bias], learning_rate=0.5), lambda: [bias])])
  p._tfrs_slices.append((torch.tensor([3, 3, 7]), torch.ones(3, 4)))
  bias.grad = torch.ones(4)
  opt.step()
  changed = (p.detach() != before).any(dim=1)
  assert changed.nonzero().reshape(-1).tolist() == [3, 7] and bool((bias != 0).all())


# ---- 6. the C entries -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  return _lib.load()


def test_c_entries_reject_bad_arguments_before_any_device_call(lib):
  """A check that ran after a launch could not return these codes on a machine without a GPU."""
  for call, code, text in rw.c_entry_argument_cases(lib):
    rc = call()
    assert rc == code and text in _lib.last_error(), (rc, code, text, _lib.last_error())
  # nothing to do is not an error, and touches nothing
  assert lib.tfrs_rowwise_adagrad_sparse(None, None, 1, 0, 8, 10, ctypes.c_void_p(256), ctypes.c_void_p(256), 0.1, None,
                                         1e-7, 1, 0, None, 0, None) == _lib.TFRS_OK
  assert lib.tfrs_rowwise_adagrad_dense(None, None, None, 0, 8, 0.1, None, 1e-7, 1, None) == _lib.TFRS_OK


def test_new_kernels_use_no_scratch_and_do_not_spill():
  """From the code object metadata of the cross-compiled sources: every ``rowwise_adagrad_*`` kernel."""
  import os
  import re
  import subprocess
  import tempfile
  from recommenders_amd.csrc import build as csrc_build
  found = {}
  for source in ("sparse_update.hip", "table_update.hip"):
    src = os.path.join(os.path.dirname(csrc_build.__file__), source)
    out = os.path.join(tempfile.mkdtemp(prefix="tfrs_rowwise_"), source + ".s")
    subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17",
                    *csrc_build.EXTRA_FLAGS.get(source, []), "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True, cwd=os.path.dirname(src))
    with open(out) as f:
      asm = f.read()
    for block in asm.split("- .agpr_count:")[1:]:
      name = re.search(r"\.name:\s+(\S+)", block).group(1)
      if "rowwise_adagrad" not in name:
        continue
      found[source] = found.get(source, 0) + 1
      assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
      assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
      assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  # sparse_update.hip: 2 learning-rate forms x (2 row-scan id types + 6 sorted forms); table_update.hip: 2 x 4 dense forms
  assert found == {"sparse_update.hip": 16, "table_update.hip": 8}
