"""``ApproxNDCGLoss``, ``ApproxMRRLoss`` and ``UniqueSoftmaxLoss`` on the MI355X (listwise_pairsum_kernel of
csrc/listwise.hip through losses.py) against the float64 restatement of tests/pairsum_restatement.py, under the
bounds derived there (any summation order; ``float_gate`` with limit eps and the restatement's yardstick), and bit for
bit where tests/test_pairsum_host.py proves the inputs exact.

Shapes: those of tests/listwise_restatement.py (B in {1, 3, 67} x L in {1, 2, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130,
256, 257, 1024}, B = 3 only at 1024): both sides of every switch of the work mapping, one and several workgroups, and
the top of the envelope."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import listwise_restatement as lw
from tests import pairsum_restatement as ps
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

GATE_FLOOR = ps.FLOOR / ps.EPS        # float_gate floors the YARDSTICK; limit eps x this = one smallest normal float
KIND_NAMES = tuple(ps.KINDS)


def _loss_class(kind_name):
  from recommenders_amd import losses
  return {"approx_ndcg": losses.ApproxNDCGLoss, "approx_mrr": losses.ApproxMRRLoss,
          "unique_softmax": losses.UniqueSoftmaxLoss}[kind_name]


def _cuda(a):
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(t):
  return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _temperature(kind_name, temperature):
  return ps.DEFAULT_TEMPERATURE[kind_name] if temperature is None else temperature


def _run(kind_name, y, s, temperature=None, weight=None, reduction="none"):
  """(loss as returned, d (sum of the returned loss) / d scores) as numpy float32; temperature None: the default."""
  yt, st = _cuda(y), _cuda(s).requires_grad_(True)
  kwargs = {} if temperature is None else {"temperature": temperature}
  out = _loss_class(kind_name)(reduction=reduction, **kwargs)(yt, st,
                                                              sample_weight=None if weight is None else _cuda(weight))
  out.sum().backward()
  return out.detach().cpu().numpy(), st.grad.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(B, L):
  seed = 100 * L + B
  return lw.make_labels(B, L, seed), lw.make_scores(B, L, seed)


@functools.lru_cache(maxsize=None)
def _reference(kind_name, B, L, temperature):
  y, s = _inputs(B, L)
  return ps.batch_loss(ps.KINDS[kind_name], y, s, _temperature(kind_name, temperature))


def _gate(name, got, entry):
  return float_gate(name, got, entry.value, entry.gate, ps.EPS, floor=GATE_FLOOR)


def _plus_zero(a):
  a = np.asarray(a)
  return not a.any() and not np.signbit(a).any()


# ---- 1. values and gradients against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
@pytest.mark.parametrize("temperature", [None, 1.0])
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_values_and_gradients_match_the_restatement(kind_name, temperature, B, L):
  y, s = _inputs(B, L)
  ref_loss, ref_grad = _reference(kind_name, B, L, temperature)
  loss, grad = _run(kind_name, y, s, temperature)
  assert loss.shape == (B,) and grad.shape == (B, L) and loss.dtype == np.float32
  el = _gate(f"pairsum.{kind_name}.loss", loss, ref_loss)
  eg = _gate(f"pairsum.{kind_name}.dscores", grad, ref_grad)
  print(f"{kind_name} T={temperature} B={B} L={L}: loss error {el / ps.EPS:.3g}, gradient error {eg / ps.EPS:.3g} "
        "of the bound")
  assert _plus_zero(grad[y < 0])


@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_list_weights_and_reductions(kind_name):
  """``sample_weight`` [B] and [B, 1] and the three reductions: the backward's scale is weight x reduction factor.  A
  weighted loss is one more rounding; a reduced one a sum of B such terms and one product."""
  B, L = 67, 33
  y, s = _inputs(B, L)
  ref_loss, ref_grad = _reference(kind_name, B, L, None)
  w = (np.random.RandomState(3).rand(B) + 0.5).astype(np.float32)
  for reduction, factor in (("none", 1.0), ("sum", 1.0), ("sum_over_batch_size", 1.0 / B)):
    for weight in (w, w[:, None]):
      loss, grad = _run(kind_name, y, s, weight=weight, reduction=reduction)
      wl = ps.scaled(ref_loss, w, 1.0)
      if reduction == "none":
        _gate(f"pairsum.{kind_name}.weighted.loss", loss, wl)
      else:
        assert loss.shape == ()
        total = float(wl.value.sum()) * factor
        b = (float(wl.bound.sum()) + (B - 1) * ps.EPS * float(np.abs(wl.value).sum())) * factor + ps.EPS * abs(total)
        _gate(f"pairsum.{kind_name}.{reduction}.loss", loss, ps.entry_from_bound(total, B, 1.0, b))
      _gate(f"pairsum.{kind_name}.weighted.dscores", grad, ps.scaled(ref_grad, (w * factor)[:, None], 2.0))
      assert _plus_zero(grad[y < 0])


# ---- 2. edges ----------------------------------------------------------------------------------------------------------
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
  s[4] = 0.75                                         # all scores equal
  y[5] = np.where(y0[5] >= 0, 0.0, -1.0)              # no positive label
  for kind_name in KIND_NAMES:
    for temperature in (None, 1.0):
      loss, grad = _run(kind_name, y, s, temperature)
      base_loss, base_grad = _run(kind_name, y0, s0, temperature)
      for b in (0, 6):                                # the neighbours do not see the degenerate lists
        assert loss.view(np.uint32)[b] == base_loss.view(np.uint32)[b]
        np.testing.assert_array_equal(grad[b].view(np.uint32), base_grad[b].view(np.uint32))
      assert np.isfinite(loss).all() and np.isfinite(grad).all()
      assert _plus_zero(loss[1]) and _plus_zero(grad[1]), kind_name
      assert _plus_zero(grad[2]), kind_name
      assert loss[2] == (0.0 if kind_name == "unique_softmax" else -1.0), kind_name
      if kind_name == "unique_softmax":               # nothing is labelled below anything: lse_i = t_i
        assert _plus_zero(loss[3]) and not grad[3].any()
      else:
        assert _plus_zero(loss[5]) and _plus_zero(grad[5]), kind_name
      ref_loss, ref_grad = ps.batch_loss(ps.KINDS[kind_name], y, s, _temperature(kind_name, temperature))
      _gate(f"pairsum.{kind_name}.degenerate.loss", loss, ref_loss)
      _gate(f"pairsum.{kind_name}.degenerate.dscores", grad, ref_grad)
      assert _plus_zero(grad[y < 0])


@pytest.mark.parametrize("L", [5, 64, 257])
def test_padded_scores_never_enter_the_arithmetic(L):
  B = 5
  y, s = lw.make_labels(B, L, 77 + L), lw.make_scores(B, L, 77 + L)
  y[0, L // 2] = -1.0
  pad = y < 0
  assert pad.any() and (~pad).any()
  base = {k: _run(k, y, s) for k in KIND_NAMES}
  for poison in (np.nan, np.inf, 1e30):
    sp = s.copy()
    sp[pad] = poison
    for kind_name in KIND_NAMES:
      loss, grad = _run(kind_name, y, sp)
      np.testing.assert_array_equal(loss.view(np.uint32), base[kind_name][0].view(np.uint32))
      np.testing.assert_array_equal(grad.view(np.uint32), base[kind_name][1].view(np.uint32))
      assert _plus_zero(grad[pad])


# ---- 3. range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 5), (67, 64), (3, 257)])
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_scores_spread_over_plus_minus_100(kind_name, B, L):
  """Saturated sigmoids, and the per-item shift of UniqueSoftmax: list 1 holds one top-labelled item at +100 (it enters
  no other item's lse) above items that all lie below -90, whose lse a shift by the list's maximum would turn into
  log 0."""
  y = lw.make_labels(B, L, 900 + L)
  s = np.random.RandomState(901 + L).uniform(-100.0, 100.0, size=(B, L)).astype(np.float32)
  s[0, 0], s[0, L - 1] = 100.0, -100.0
  s[1] = np.random.RandomState(902 + L).uniform(-100.0, -90.0, size=L).astype(np.float32)
  s[1, 0], y[1, 0] = 100.0, 5.0
  for temperature in (None, 1.0):
    loss, grad = _run(kind_name, y, s, temperature)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    ref_loss, ref_grad = ps.batch_loss(ps.KINDS[kind_name], y, s, _temperature(kind_name, temperature))
    _gate(f"pairsum.{kind_name}.range.loss", loss, ref_loss)
    _gate(f"pairsum.{kind_name}.range.dscores", grad, ref_grad)


@pytest.mark.parametrize("B,L", [(3, 5), (67, 64), (3, 257)])
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_temperature_one_thousandth(kind_name, B, L):
  y, s = _inputs(B, L)
  loss, grad = _run(kind_name, y, s, 1e-3)
  assert np.isfinite(loss).all() and np.isfinite(grad).all()
  ref_loss, ref_grad = ps.batch_loss(ps.KINDS[kind_name], y, s, 1e-3)
  _gate(f"pairsum.{kind_name}.cold.loss", loss, ref_loss)
  _gate(f"pairsum.{kind_name}.cold.dscores", grad, ref_grad)


# ---- 4. ApproxMRR, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", ps.MRR_EXACT_TEMPERATURES)
@pytest.mark.parametrize("n", ps.MRR_EXACT_N)
def test_approx_mrr_on_exact_inputs_is_bit_equal(n, temperature):
  """All valid scores of a list equal, labels in {0, 1} with one or two ones, n + 1 a power of two, power-of-two
  temperature and list weights: every partial sum of every order is an exact float32
  (tests/test_pairsum_host.py: test_approx_mrr_exact_inputs_are_exact proves it for each of these inputs), so the
  kernel's loss and gradient equal the float64 restatement rounded to float32 bit for bit."""
  y, s, w = ps.mrr_exact_inputs(n)
  ref_loss, ref_grad = ps.batch_loss(ps.APPROX_MRR, y, s, temperature)
  loss, grad = _run("approx_mrr", y, s, temperature, weight=w)
  w64 = w.astype(np.float64)
  np.testing.assert_array_equal(ref_loss.value, -2.0 / (n + 1))
  np.testing.assert_array_equal(loss.view(np.uint32), (ref_loss.value * w64).astype(np.float32).view(np.uint32))
  np.testing.assert_array_equal(grad.view(np.uint32),
                                (ref_grad.value * w64[:, None]).astype(np.float32).view(np.uint32))
  assert _plus_zero(grad[y < 0]) and (n == 1 or grad.any())


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(67, 5), (67, 64), (67, 130), (3, 1024)])
def test_two_calls_give_identical_bits(B, L):
  y, s = _inputs(B, L)
  for kind_name in KIND_NAMES:
    a, b = _run(kind_name, y, s), _run(kind_name, y, s)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- 6. no L^2 memory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_losses_allocate_no_pair_matrix(kind_name):
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


# ---- 7. captured step --------------------------------------------------------------------------------------------------
def test_captured_step_replays_the_eager_trajectory_bit_for_bit():
  import recommenders_amd as tfrs
  B, L = 48, 5

  class Ranker(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.items = tfrs.layers.embedding.Embedding(500, 16)
      self.score = tfrs.layers.blocks.Dense(1)
      self.ndcg = tfrs.metrics.NDCGMetric(topn=5)
      self.mrr = tfrs.metrics.MRRMetric()
      self.task = tfrs.tasks.Ranking(loss=tfrs.losses.ApproxNDCGLoss(), metrics=[self.ndcg, self.mrr])

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
    assert float(le["loss"]) == float(lg["loss"]) and float(le["loss"]) < 0.0
    assert float(le["ndcg_metric"]) == float(lg["ndcg_metric"])
    assert float(le["mrr_metric"]) == float(lg["mrr_metric"])
  for a, b, s0 in zip(eager.parameters(), graphed.parameters(), start):
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not torch.equal(a, s0)
  for name in ("ndcg", "mrr"):
    assert float(getattr(eager, name).result()) == float(getattr(graphed, name).result())
    assert 0.0 < float(getattr(graphed, name).result()) <= 1.0


# ---- 8. C entries ------------------------------------------------------------------------------------------------------
def test_c_entries_validate_and_skip_empty_batches():
  from recommenders_amd import _lib
  lib = _lib.load()
  buf = torch.zeros(64, device="cuda")
  p, stream = _lib.ptr(buf), _lib.current_stream()
  null = ctypes.c_void_p(0)
  calls = {
      "kind 3": lambda: lib.tfrs_listwise_pairsum_fwd(3, p, p, 2, 5, 1.0, p, stream),
      "kind -1": lambda: lib.tfrs_listwise_pairsum_bwd(-1, p, p, 2, 5, 1.0, p, p, stream),
      "temperature 0": lambda: lib.tfrs_listwise_pairsum_fwd(0, p, p, 2, 5, 0.0, p, stream),
      "temperature -1": lambda: lib.tfrs_listwise_pairsum_bwd(1, p, p, 2, 5, -1.0, p, p, stream),
      "temperature nan": lambda: lib.tfrs_listwise_pairsum_fwd(2, p, p, 2, 5, float("nan"), p, stream),
      "temperature inf": lambda: lib.tfrs_listwise_pairsum_bwd(2, p, p, 2, 5, float("inf"), p, p, stream),
      "temperature 1e-46": lambda: lib.tfrs_listwise_pairsum_fwd(0, p, p, 2, 5, 1e-46, p, stream),
      "temperature 1e-39": lambda: lib.tfrs_listwise_pairsum_fwd(0, p, p, 2, 5, 1e-39, p, stream),
      "len 0": lambda: lib.tfrs_listwise_pairsum_fwd(0, p, p, 2, 0, 1.0, p, stream),
      "len 1025": lambda: lib.tfrs_listwise_pairsum_bwd(2, p, p, 2, 1025, 1.0, p, p, stream),
      "NULL labels": lambda: lib.tfrs_listwise_pairsum_fwd(0, null, p, 2, 5, 1.0, p, stream),
      "NULL loss": lambda: lib.tfrs_listwise_pairsum_fwd(1, p, p, 2, 5, 1.0, null, stream),
      "NULL scale": lambda: lib.tfrs_listwise_pairsum_bwd(1, p, p, 2, 5, 1.0, null, p, stream),
      "NULL dscores": lambda: lib.tfrs_listwise_pairsum_bwd(2, p, p, 2, 5, 1.0, p, null, stream),
  }
  for what, call in calls.items():
    assert call() == _lib.TFRS_EINVAL, what
    assert "listwise_pairsum" in _lib.last_error(), what
  for kind in range(3):
    assert lib.tfrs_listwise_pairsum_fwd(kind, null, null, 0, 5, 0.1, null, stream) == _lib.TFRS_OK
    assert lib.tfrs_listwise_pairsum_bwd(kind, null, null, 0, 5, 0.1, null, null, stream) == _lib.TFRS_OK
  torch.cuda.synchronize()
  assert not buf.any()
  # the host classes on an empty batch: empty / zero results, gradients flow
  from recommenders_amd import losses
  empty_y, empty_s = torch.zeros(0, 5, device="cuda"), torch.zeros(0, 5, device="cuda", requires_grad=True)
  assert losses.ApproxMRRLoss(reduction="none")(empty_y, empty_s).shape == (0,)
  out = losses.UniqueSoftmaxLoss()(empty_y, empty_s)
  out.backward()
  assert float(out.detach()) == 0.0 and empty_s.grad.shape == (0, 5)
