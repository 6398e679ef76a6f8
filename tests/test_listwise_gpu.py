"""The listwise ranking losses and ``NDCGMetric`` on the MI355X (csrc/listwise.hip through losses.py and
metrics/listwise.py) against the float64 restatement of tests/listwise_restatement.py, under the bounds derived there
(any summation order; ``float_gate`` with limit eps and the restatement's yardstick), and bit for bit where
tests/test_listwise_host.py proves the inputs exact.

Shapes: B in {1, 3, 67} x L in {1, 2, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 256, 257, 1024} (B = 3 only at 1024):
both sides of every switch of the work mapping (8 / 16 / 32 / 64 lanes per list, then a workgroup per list with 1 .. 4
items per thread and sort widths 128 .. 1024), one and several workgroups, and the top of the envelope."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import listwise_restatement as lw
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

GATE_FLOOR = lw.FLOOR / lw.EPS        # float_gate floors the YARDSTICK; limit eps x this = one smallest normal float
KIND_NAMES = tuple(lw.KINDS)


def _loss_class(kind_name):
  from recommenders_amd import losses
  return {"softmax": losses.SoftmaxLoss, "pairwise_logistic": losses.PairwiseLogisticLoss,
          "pairwise_hinge": losses.PairwiseHingeLoss, "list_mle": losses.ListMLELoss}[kind_name]


def _cuda(a):
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(t):
  return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(kind_name, y, s, weight=None, reduction="none"):
  """(loss as returned, d (sum of the returned loss) / d scores) as numpy float32."""
  yt, st = _cuda(y), _cuda(s).requires_grad_(True)
  out = _loss_class(kind_name)(reduction=reduction)(yt, st, sample_weight=None if weight is None else _cuda(weight))
  out.sum().backward()
  return out.detach().cpu().numpy(), st.grad.detach().cpu().numpy()


def _ndcg_lists(y, s, topn):
  """Per-list NDCG and counted flags straight from the C entry."""
  from recommenders_amd import _lib
  yt, st = _cuda(y), _cuda(s)
  out = torch.full((2, y.shape[0]), -7.0, device="cuda")
  _lib.check(_lib.load().tfrs_listwise_ndcg(_lib.ptr(yt), _lib.ptr(st), y.shape[0], y.shape[1], 0 if topn is None else topn,
                                            _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.current_stream()))
  return out[0].cpu().numpy(), out[1].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(B, L):
  seed = 100 * L + B
  return lw.make_labels(B, L, seed), lw.make_scores(B, L, seed)


@functools.lru_cache(maxsize=None)
def _reference(kind_name, B, L):
  y, s = _inputs(B, L)
  return lw.batch_loss(lw.KINDS[kind_name], y, s)


def _gate(name, got, entry):
  return float_gate(name, got, entry.value, entry.gate, lw.EPS, floor=GATE_FLOOR)


def _padded_gradients_are_plus_zero(y, grad):
  pad = y < 0
  assert not grad[pad].any() and not np.signbit(grad[pad]).any()


# ---- 1. values and gradients against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_values_and_gradients_match_the_restatement(kind_name, B, L):
  y, s = _inputs(B, L)
  ref_loss, ref_grad = _reference(kind_name, B, L)
  loss, grad = _run(kind_name, y, s)
  assert loss.shape == (B,) and grad.shape == (B, L) and loss.dtype == np.float32
  el = _gate(f"listwise.{kind_name}.loss", loss, ref_loss)
  eg = _gate(f"listwise.{kind_name}.dscores", grad, ref_grad)
  print(f"{kind_name} B={B} L={L}: loss error {el / lw.EPS:.3g}, gradient error {eg / lw.EPS:.3g} of the bound")
  _padded_gradients_are_plus_zero(y, grad)


@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_list_weights_and_reductions(kind_name):
  """``sample_weight`` [B] and [B, 1] and the three reductions: the backward's scale is weight x reduction factor."""
  B, L = 67, 33
  y, s = _inputs(B, L)
  ref_loss, ref_grad = _reference(kind_name, B, L)
  w = (np.random.RandomState(3).rand(B) + 0.5).astype(np.float32)
  for reduction, factor in (("none", 1.0), ("sum", 1.0), ("sum_over_batch_size", 1.0 / B)):
    for weight in (w, w[:, None]):
      loss, grad = _run(kind_name, y, s, weight=weight, reduction=reduction)
      wl = lw.Entry(ref_loss.value * w, ref_loss.n, ref_loss.yard * w, ref_loss.u + 1.0)
      if reduction == "none":
        _gate(f"listwise.{kind_name}.weighted.loss", loss, wl)
      else:       # one more sum over the B lists
        tot = lw.Entry(wl.value.sum() * factor, ref_loss.n.sum(), wl.yard.sum() * factor, ref_loss.u + 2.0)
        assert loss.shape == ()
        _gate(f"listwise.{kind_name}.{reduction}.loss", loss, tot)
      sc = (w * factor)[:, None]
      _gate(f"listwise.{kind_name}.weighted.dscores", grad,
            lw.Entry(ref_grad.value * sc, ref_grad.n, ref_grad.yard * sc, ref_grad.u + 2.0))


# ---- 2. hinge, exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
def test_hinge_on_exact_inputs_is_bit_equal(B, L):
  """Scores on the 1/4 grid in [-2, 2], power-of-two list weights, reduction "sum": every partial sum of every order
  is an exact float32 (tests/test_listwise_host.py: test_hinge_exact_inputs_are_exact proves it for each of these
  shapes), so the kernel's loss and gradient equal the float64 restatement rounded to float32 bit for bit."""
  y, s, w = lw.hinge_inputs(B, L)
  ref_loss, ref_grad = lw.batch_loss(lw.PAIRWISE_HINGE, y, s)
  loss, grad = _run("pairwise_hinge", y, s, weight=w, reduction="sum")
  want = np.float32(np.sum(ref_loss.value * w.astype(np.float64)))
  assert float(want) == float(np.sum(ref_loss.value * w.astype(np.float64)))
  np.testing.assert_array_equal(loss, want)
  np.testing.assert_array_equal(grad, (ref_grad.value * w.astype(np.float64)[:, None]).astype(np.float32))
  _padded_gradients_are_plus_zero(y, grad)


# ---- 3. NDCG -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
def test_ndcg_matches_the_restatement(B, L):
  """Scores on a grid (no rounding can flip an order; ties in scores and in labels by construction), every topn,
  weighted and unweighted: the per-list values of the C entry, then two updates, ``result`` and ``reset_states``."""
  from recommenders_amd import metrics
  seed = 300 * L + B
  batches = [(lw.make_labels(B, L, seed + k), lw.make_grid_scores(B, L, seed + k, step=0.5, lim=3.0)) for k in (0, 1)]
  for y, s in batches:                 # planted ties: two equal scores, and two equal labels that both count
    if L >= 2:
      s[:, 1] = s[:, 0]
    if L >= 3:
      y[:, 2] = y[:, 0] = 2.0
  weights = [(np.random.RandomState(seed + k).rand(B) + 0.25).astype(np.float32) for k in (0, 1)]
  for topn in (None, 1, 10, 2000):
    y, s = batches[0]
    got, counted = _ndcg_lists(y, s, topn)
    want, want_counted, bnd = lw.batch_ndcg(y, s, topn)
    np.testing.assert_array_equal(counted, want_counted)
    float_gate("listwise.ndcg.lists", got, want, bnd / lw.EPS, lw.EPS, floor=GATE_FLOOR)
    assert not got[want_counted == 0].any()
    for weighted in (False, True):
      metric = metrics.NDCGMetric(topn=topn)
      assert float(metric.result()) == 0.0
      updates = []
      for k, (y, s) in enumerate(batches):
        w = weights[k] if weighted else None
        metric.update_state(_cuda(y), _cuda(s), sample_weight=None if w is None else _cuda(w[:, None] if k else w))
        updates.append((y, s, w))
      value, bnd_result = lw.ndcg_result(updates, topn)
      got_result = float(metric.result())
      assert abs(got_result - value) <= bnd_result + lw.FLOOR, (topn, weighted, got_result, value, bnd_result)
      metric.reset_states()
      assert float(metric.result()) == 0.0
      metric.update_state(_cuda(batches[0][0]), _cuda(batches[0][1]))
      first, _ = lw.ndcg_result([(batches[0][0], batches[0][1], None)], topn)
      assert float(metric.result()) == pytest.approx(first, abs=1e-5)
      metric.reset_state()
      assert float(metric.result()) == 0.0


# ---- 4. degenerate lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 130])
def test_degenerate_lists_inside_a_normal_batch(L):
  B = 7
  y0, s0 = lw.make_labels(B, L, 41 + L), lw.make_scores(B, L, 41 + L)
  y0[:, 0] = np.maximum(y0[:, 0], 1.0)                 # every normal list has a gain
  y, s = y0.copy(), s0.copy()
  y[1] = -1.0                                         # all padding
  y[2] = -1.0
  y[2, L // 2] = 3.0                                  # one valid item
  y[3] = np.where(y0[3] >= 0, 2.0, -1.0)              # all labels equal
  y[3, 0] = 2.0
  s[4] = 0.75                                         # all scores equal
  y[5] = np.where(y0[5] >= 0, 0.0, -1.0)              # labels all zero
  n_pairs4 = sum(1 for i in range(L) for j in range(L) if y[4, j] >= 0 and y[4, i] > y[4, j])
  for kind_name in KIND_NAMES:
    loss, grad = _run(kind_name, y, s)
    base_loss, base_grad = _run(kind_name, y0, s0)
    for b in (0, 6):                                  # the neighbours do not see the degenerate lists
      assert loss.view(np.uint32)[b] == base_loss.view(np.uint32)[b]
      np.testing.assert_array_equal(grad[b].view(np.uint32), base_grad[b].view(np.uint32))
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    for b in (1, 2):
      assert loss[b] == 0.0 and not grad[b].any(), (kind_name, b)
    if kind_name.startswith("pairwise"):
      assert loss[3] == 0.0 and not grad[3].any()
      assert loss[5] == 0.0 and not grad[5].any()
    if kind_name == "pairwise_hinge":
      assert loss[4] == float(n_pairs4)
    if kind_name == "softmax":
      assert loss[5] == 0.0 and not grad[5].any()
    ref_loss, ref_grad = lw.batch_loss(lw.KINDS[kind_name], y, s)
    _gate(f"listwise.{kind_name}.degenerate.loss", loss, ref_loss)
    _gate(f"listwise.{kind_name}.degenerate.dscores", grad, ref_grad)
  got, counted = _ndcg_lists(y, s, None)
  base, _ = _ndcg_lists(y0, s0, None)
  assert list(counted) == [1.0, 0.0, 1.0, 1.0, float(y[4].max() > 0), 0.0, 1.0]
  assert got[1] == 0.0 and got[5] == 0.0 and got[2] == 1.0 and got[3] == 1.0
  np.testing.assert_array_equal(got[[0, 6]].view(np.uint32), base[[0, 6]].view(np.uint32))


# ---- 5. padding is select, not multiply ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 257])
def test_padded_scores_never_enter_the_arithmetic(L):
  B = 5
  y, s = lw.make_labels(B, L, 77 + L), lw.make_scores(B, L, 77 + L)
  y[0, L // 2] = -1.0
  pad = y < 0
  assert pad.any() and (~pad).any()
  base = {k: _run(k, y, s) for k in KIND_NAMES}
  base_ndcg = _ndcg_lists(y, s, 10)
  for poison in (np.nan, np.inf, 1e30):
    sp = s.copy()
    sp[pad] = poison
    for kind_name in KIND_NAMES:
      loss, grad = _run(kind_name, y, sp)
      np.testing.assert_array_equal(loss.view(np.uint32), base[kind_name][0].view(np.uint32))
      np.testing.assert_array_equal(grad.view(np.uint32), base[kind_name][1].view(np.uint32))
      _padded_gradients_are_plus_zero(y, grad)
    got = _ndcg_lists(y, sp, 10)
    np.testing.assert_array_equal(got[0].view(np.uint32), base_ndcg[0].view(np.uint32))
    np.testing.assert_array_equal(got[1], base_ndcg[1])


# ---- 6. range --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 5), (67, 64), (3, 257)])
@pytest.mark.parametrize("kind_name", ["softmax", "pairwise_logistic", "list_mle"])
def test_scores_spread_over_plus_minus_80(kind_name, B, L):
  y = lw.make_labels(B, L, 900 + L)
  s = np.random.RandomState(901 + L).uniform(-80.0, 80.0, size=(B, L)).astype(np.float32)
  s[0, 0], s[0, L - 1] = 80.0, -80.0
  loss, grad = _run(kind_name, y, s)
  assert np.isfinite(loss).all() and np.isfinite(grad).all()
  ref_loss, ref_grad = lw.batch_loss(lw.KINDS[kind_name], y, s)
  _gate(f"listwise.{kind_name}.range.loss", loss, ref_loss)
  _gate(f"listwise.{kind_name}.range.dscores", grad, ref_grad)


# ---- 7. reproducibility ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(67, 5), (67, 64), (67, 130), (3, 1024)])
def test_two_calls_give_identical_bits(B, L):
  y, s = _inputs(B, L)
  for kind_name in KIND_NAMES:
    a, b = _run(kind_name, y, s), _run(kind_name, y, s)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
  a, b = _ndcg_lists(y, s, 10), _ndcg_lists(y, s, 10)
  np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ---- 8. no L^2 memory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", ["pairwise_logistic", "pairwise_hinge"])
def test_pairwise_losses_allocate_no_pair_matrix(kind_name):
  """B = 64, L = 1024: a [B, L, L] float32 temporary would be 256 MiB; forward + backward may add 8 B L 4 bytes + 1 MiB."""
  B, L = 64, 1024
  yt = _cuda(lw.make_labels(B, L, 5))
  st = _cuda(lw.make_scores(B, L, 5)).requires_grad_(True)
  loss_fn = _loss_class(kind_name)()
  loss_fn(yt, st).backward()        # (library load, lazy initialisation)
  st.grad = None
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  loss_fn(yt, st).backward()
  torch.cuda.synchronize()
  added = torch.cuda.max_memory_allocated() - before
  print(f"{kind_name}: peak over the inputs {added} bytes")
  assert added <= 8 * B * L * 4 + (1 << 20), added
  assert st.grad is not None and bool(st.grad.abs().sum() > 0)


# ---- 9. captured step --------------------------------------------------------------------------------------------------
def test_captured_step_replays_the_eager_trajectory_bit_for_bit():
  import recommenders_amd as tfrs
  B, L = 48, 5

  class Ranker(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.items = tfrs.layers.embedding.Embedding(500, 16)
      self.score = tfrs.layers.blocks.Dense(1)
      self.ndcg = tfrs.metrics.NDCGMetric(topn=5)
      self.task = tfrs.tasks.Ranking(loss=tfrs.losses.PairwiseLogisticLoss(), metrics=[self.ndcg])

    def compute_loss(self, inputs, training=False):
      ids = inputs["items"]
      scores = self.score(self.items(ids.reshape(-1))).reshape(ids.shape)
      return self.task(labels=inputs["labels"], predictions=scores)

  def make():
    torch.manual_seed(11)
    m = Ranker().cuda()
    with torch.no_grad():        # (builds the lazily created Dense kernel)
      m.score(m.items(torch.zeros(4, dtype=torch.int64, device="cuda")))
    m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.1))
    return m

  rng = np.random.RandomState(12)
  batches = [{"items": _cuda(rng.randint(0, 500, size=(B, L)).astype(np.int64)),
              "labels": _cuda(lw.make_labels(B, L, 50 + k))} for k in range(3)]
  eager, graphed = make(), make()
  assert len(list(eager.parameters())) == 3
  step = graphed.make_graphed_train_step(batches[0])
  for a, b in zip(eager.parameters(), graphed.parameters()):      # warm-up rolled back
    np.testing.assert_array_equal(_bits(a), _bits(b))
  start = [p.detach().clone() for p in eager.parameters()]
  for batch in batches:
    le, lg = eager.train_step(batch), step(batch)
    assert float(le["loss"]) == float(lg["loss"])
    assert float(le["ndcg_metric"]) == float(lg["ndcg_metric"])
  for a, b, s0 in zip(eager.parameters(), graphed.parameters(), start):
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not torch.equal(a, s0)
  for name in ("_total", "_count"):
    np.testing.assert_array_equal(_bits(getattr(eager.ndcg, name)), _bits(getattr(graphed.ndcg, name)))
  assert float(eager.ndcg._count) == float(sum(int((b["labels"].max(dim=1).values > 0).sum()) for b in batches))
  assert 0.0 < float(graphed.ndcg.result()) <= 1.0


# ---- 10. C entries -----------------------------------------------------------------------------------------------------
def test_c_entries_validate_and_skip_empty_batches():
  from recommenders_amd import _lib
  lib = _lib.load()
  buf = torch.zeros(64, device="cuda")
  p, stream = _lib.ptr(buf), _lib.current_stream()
  null = ctypes.c_void_p(0)
  calls = {
      "NULL labels": lambda: lib.tfrs_listwise_loss_fwd(0, null, p, 2, 5, p, stream),
      "NULL loss": lambda: lib.tfrs_listwise_loss_fwd(0, p, p, 2, 5, null, stream),
      "NULL scale": lambda: lib.tfrs_listwise_loss_bwd(1, p, p, 2, 5, null, p, stream),
      "NULL counted": lambda: lib.tfrs_listwise_ndcg(p, p, 2, 5, 0, p, null, stream),
      "len 0": lambda: lib.tfrs_listwise_loss_fwd(0, p, p, 2, 0, p, stream),
      "len 1025": lambda: lib.tfrs_listwise_loss_bwd(2, p, p, 2, 1025, p, p, stream),
      "len 1025 ndcg": lambda: lib.tfrs_listwise_ndcg(p, p, 2, 1025, 0, p, p, stream),
      "kind 4": lambda: lib.tfrs_listwise_loss_fwd(4, p, p, 2, 5, p, stream),
      "kind -1": lambda: lib.tfrs_listwise_loss_bwd(-1, p, p, 2, 5, p, p, stream),
      "topn -1": lambda: lib.tfrs_listwise_ndcg(p, p, 2, 5, -1, p, p, stream),
  }
  for what, call in calls.items():
    assert call() == _lib.TFRS_EINVAL, what
    assert "listwise" in _lib.last_error(), what
  assert lib.tfrs_listwise_loss_fwd(0, null, null, 0, 5, null, stream) == _lib.TFRS_OK
  assert lib.tfrs_listwise_loss_bwd(3, null, null, 0, 5, null, null, stream) == _lib.TFRS_OK
  assert lib.tfrs_listwise_ndcg(null, null, 0, 5, 3, null, null, stream) == _lib.TFRS_OK
  torch.cuda.synchronize()
  assert not buf.any()
  # the host classes on an empty batch: empty / zero results, gradients flow
  from recommenders_amd import losses, metrics
  empty_y, empty_s = torch.zeros(0, 5, device="cuda"), torch.zeros(0, 5, device="cuda", requires_grad=True)
  assert losses.ListMLELoss(reduction="none")(empty_y, empty_s).shape == (0,)
  out = losses.SoftmaxLoss()(empty_y, empty_s)
  out.backward()
  assert float(out.detach()) == 0.0 and empty_s.grad.shape == (0, 5)
  metric = metrics.NDCGMetric()
  metric.update_state(empty_y, empty_s.detach())
  assert float(metric.result()) == 0.0
