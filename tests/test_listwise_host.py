"""Listwise ranking losses and NDCG without a GPU: the float64 restatement (tests/listwise_restatement.py) against
closed forms and finite differences, its padding behaviour, the exactness condition that makes the GPU hinge test's
bit-equality legitimate, and the host-side validation of the product classes and of the C entries (which reject bad
arguments before any device call)."""

import math

import numpy as np
import pytest
import torch

from tests import listwise_restatement as lw

SMOOTH = (lw.SOFTMAX, lw.PAIRWISE_LOGISTIC, lw.LIST_MLE)
ALL_KINDS = SMOOTH + (lw.PAIRWISE_HINGE,)


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(0.3, -1.2), (-2.0, 1.5), (0.0, 0.0), (40.0, -40.0), (-40.0, 40.0)])
def test_two_items_smooth_losses_are_log1p_exp(a, b):
  """y = (1, 0), s = (a, b): softmax, pairwise logistic and ListMLE all equal log(1 + exp(b - a)) (lse - s cancels in
  the softmax and ListMLE forms, so the float64 tolerance is absolute in the size of the scores)."""
  tol = 1e-14 * max(1.0, abs(a), abs(b))
  want = max(b - a, 0.0) + math.log1p(math.exp(-abs(b - a)))
  for kind in SMOOTH:
    loss, grad = lw.list_loss(kind, [1.0, 0.0], [a, b])
    assert loss.value == pytest.approx(want, rel=1e-13, abs=tol)
    sig = 1.0 / (1.0 + math.exp(a - b))       # d/da = -sig, d/db = +sig
    np.testing.assert_allclose(grad.value, [-sig, sig], rtol=1e-12, atol=tol)


def test_hinge_closed_forms():
  loss, grad = lw.list_loss(lw.PAIRWISE_HINGE, [1.0, 0.0], [0.25, 0.5])
  assert loss.value == 1.25 and list(grad.value) == [-1.0, 1.0]
  loss, grad = lw.list_loss(lw.PAIRWISE_HINGE, [1.0, 0.0], [2.0, 0.5])      # margin met: x = 1.5 >= 1
  assert loss.value == 0.0 and list(grad.value) == [0.0, 0.0]
  # three items, labels 2 > 1 > 0, scores 0, 0, 0: three pairs at x = 0 -> 3; the middle item's gradient cancels
  loss, grad = lw.list_loss(lw.PAIRWISE_HINGE, [2.0, 1.0, 0.0], [0.0, 0.0, 0.0])
  assert loss.value == 3.0 and list(grad.value) == [-2.0, 0.0, 2.0]


def test_ndcg_by_hand():
  # L = 2: labels (0, 1), the relevant item ranked second: DCG = 1 / log2(3), IDCG = 1
  v, c, _ = lw.list_ndcg([0.0, 1.0], [0.9, 0.1])
  assert c == 1.0 and v == pytest.approx(1.0 / math.log2(3.0), rel=1e-15)
  # ... and cut at 1 it scores nothing, but still counts (IDCG@1 = 1)
  assert lw.list_ndcg([0.0, 1.0], [0.9, 0.1], topn=1)[:2] == (0.0, 1.0)
  # L = 3: labels (3, 1, 2), scores rank the items 1, 2, 0
  y, s = [3.0, 1.0, 2.0], [0.1, 0.9, 0.5]
  dcg = 1.0 / 1.0 + 3.0 / math.log2(3.0) + 7.0 / 2.0
  idcg = 7.0 / 1.0 + 3.0 / math.log2(3.0) + 1.0 / 2.0
  assert lw.list_ndcg(y, s)[0] == pytest.approx(dcg / idcg, rel=1e-15)
  assert lw.list_ndcg(y, s, topn=2)[0] == pytest.approx((1.0 + 3.0 / math.log2(3.0)) / (7.0 + 3.0 / math.log2(3.0)),
                                                         rel=1e-15)
  assert lw.list_ndcg(y, s, topn=2000)[0] == lw.list_ndcg(y, s)[0]
  # ties: equal scores keep the position order; equal labels likewise
  assert lw.score_order([1.0, 2.0, 0.0], [0.5, 0.5, 0.5]) == [0, 1, 2]
  assert lw.label_order([1.0, 2.0, 1.0, -1.0]) == [1, 0, 2]


# ---- gradients against central finite differences --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_restatement_gradients_match_finite_differences(kind):
  rng = np.random.RandomState(5 + kind)
  for L in (1, 2, 5, 11):
    y = rng.randint(-1, 5, size=L).astype(np.float64)
    s = rng.randn(L) * 2.0
    if kind == lw.PAIRWISE_HINGE:      # away from the kink: differences are multiples of 0.4 (0.8, 1.2, ...) +- 0.1
      s = np.round(s / 0.4) * 0.4 + rng.uniform(-0.05, 0.05, size=L)
      assert all(abs(1.0 - (s[i] - s[j])) > 0.05 for i in range(L) for j in range(L) if i != j)
    _, grad = lw.list_loss(kind, y, s)
    h = 1e-5
    for k in range(L):
      sp, sm = s.copy(), s.copy()
      sp[k] += h
      sm[k] -= h
      fd = (lw.list_loss(kind, y, sp)[0].value - lw.list_loss(kind, y, sm)[0].value) / (2.0 * h)
      assert grad.value[k] == pytest.approx(fd, rel=1e-6, abs=1e-7), (kind, L, k)
      if y[k] < 0:
        assert grad.value[k] == 0.0


# ---- padding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_moving_a_pad_changes_nothing_at_the_valid_items(kind):
  y = [2.0, 0.0, 3.0, 1.0, 1.0]
  s = [0.3, -1.0, 0.7, 2.0, -0.4]
  base_loss, base_grad = lw.list_loss(kind, y, s)
  for at in range(len(y) + 1):
    yp = y[:at] + [-1.0] + y[at:]
    sp = s[:at] + [123.0] + s[at:]
    loss, grad = lw.list_loss(kind, yp, sp)
    assert loss.value == pytest.approx(base_loss.value, rel=1e-14)
    np.testing.assert_allclose(np.delete(grad.value, at), base_grad.value, rtol=1e-13)
    assert grad.value[at] == 0.0
    for topn in (None, 2):
      assert lw.list_ndcg(yp, sp, topn)[0] == pytest.approx(lw.list_ndcg(y, s, topn)[0], rel=1e-14)


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_degenerate_lists_give_zero(kind):
  loss, grad = lw.list_loss(kind, [-1.0, -1.0, -1.0], [1.0, 2.0, 3.0])
  assert loss.value == 0.0 and not grad.value.any()
  if kind in (lw.PAIRWISE_LOGISTIC, lw.PAIRWISE_HINGE):          # P is empty: all labels equal
    loss, grad = lw.list_loss(kind, [2.0, 2.0, -1.0, 2.0], [1.0, 2.0, 9.0, 3.0])
    assert loss.value == 0.0 and not grad.value.any()
  if kind == lw.SOFTMAX:                                          # sum of labels zero
    loss, grad = lw.list_loss(kind, [0.0, 0.0, -1.0], [1.0, 2.0, 3.0])
    assert loss.value == 0.0 and not grad.value.any()


def test_ndcg_excludes_lists_without_gain():
  assert lw.list_ndcg([0.0, 0.0, -1.0], [1.0, 2.0, 3.0])[:2] == (0.0, 0.0)
  assert lw.list_ndcg([-1.0, -1.0], [1.0, 2.0])[:2] == (0.0, 0.0)
  y = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
  s = np.array([[1.0, 2.0], [0.9, 0.1], [0.9, 0.1]])
  v, _ = lw.ndcg_result([(y, s, None)])
  assert v == pytest.approx((1.0 / math.log2(3.0) + 1.0) / 2.0, rel=1e-15)      # the first list does not count
  v, _ = lw.ndcg_result([(y, s, [5.0, 1.0, 3.0])])
  assert v == pytest.approx((1.0 / math.log2(3.0) + 3.0) / 4.0, rel=1e-15)
  assert lw.ndcg_result([(y[:1], s[:1], None)]) == (0.0, 0.0)


# ---- the exact cases of the GPU hinge test ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
def test_hinge_exact_inputs_are_exact(B, L):
  """Every (B, L) the GPU hinge test compares bit for bit: scores on the 1/4 grid in [-2, 2], power-of-two weights,
  and the total in grid steps below 2^24 (tests/listwise_restatement.py: hinge_exact_steps says why that suffices)."""
  y, s, w = lw.hinge_inputs(B, L)
  assert np.all(s * 4.0 == np.round(s * 4.0)) and np.abs(s).max() <= 2.0
  assert np.all(np.log2(w) == np.round(np.log2(w)))
  assert (y == -1.0).any() or L < 64
  ok, steps = lw.hinge_exact_steps(y, s, w)
  assert ok, f"B={B} L={L}: {steps} steps of {lw.HINGE_STEP} x min weight is not below 2^24"


def test_hinge_exact_condition_rejects_what_it_should():
  y = np.array([[1.0, 0.0]])
  assert lw.hinge_exact_steps(y, np.array([[0.25, 0.5]]), np.array([1.0])) == (True, 5)
  assert not lw.hinge_exact_steps(y, np.array([[0.3, 0.5]]), np.array([1.0]))[0]          # off the grid
  assert not lw.hinge_exact_steps(np.array([[1.0, 0.0], [1.0, 0.0]]), np.zeros((2, 2)),
                                  np.array([1.0, 2.0 ** 23]))[0]                            # 4 + 2^25 steps


# ---- validation ------------------------------------------------------------------------------------------------------
def _classes():
  from recommenders_amd import losses
  return (losses.SoftmaxLoss, losses.PairwiseLogisticLoss, losses.PairwiseHingeLoss, losses.ListMLELoss)


def test_constructors_and_shapes_are_validated_before_the_device():
  from recommenders_amd import losses, metrics
  assert losses.MAX_LIST_LEN == lw.MAX_LIST_LEN == 1024
  y, s = torch.zeros(4, 5), torch.zeros(4, 5)
  for cls in _classes():
    with pytest.raises(ValueError, match="reduction"):
      cls(reduction="mean")
    assert cls(reduction="auto").reduction == "sum_over_batch_size"
    loss = cls()
    with pytest.raises(ValueError, match="per list"):
      loss(y, s, sample_weight=torch.ones(4, 5))
    with pytest.raises(ValueError, match=r"\[batch, list\]"):
      loss(torch.zeros(5), torch.zeros(5))
    with pytest.raises(ValueError, match=r"\[batch, list\]"):
      loss(torch.zeros(4, 5), torch.zeros(4, 6))
    with pytest.raises(ValueError, match="MAX_LIST_LEN"):
      loss(torch.zeros(2, 1025), torch.zeros(2, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      loss(y, s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      loss(y, s, sample_weight=torch.ones(4, 1))
  assert metrics.NDCGMetric().name == "ndcg_metric" and metrics.NDCGMetric().topn is None
  for bad in (0, -3, 2.5):
    with pytest.raises(ValueError, match="topn"):
      metrics.NDCGMetric(topn=bad)
  m = metrics.NDCGMetric(topn=5)
  with pytest.raises(ValueError, match="per list"):
    m.update_state(y, s, sample_weight=torch.ones(4, 5))
  with pytest.raises(ValueError, match="MAX_LIST_LEN"):
    m.update_state(torch.zeros(2, 1025), torch.zeros(2, 1025))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    m.update_state(y, s)
  assert float(m.result()) == 0.0
  m.reset_states()
  m.reset_state()


def test_c_entries_reject_bad_arguments_before_any_device_call():
  import ctypes
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  lib = _lib.load()
  p = ctypes.c_void_p(256)       # never dereferenced: every call below returns before a launch
  fwd = lambda kind, y, s, n, l, out: lib.tfrs_listwise_loss_fwd(kind, y, s, n, l, out, None)
  bwd = lambda kind, y, s, n, l, sc, out: lib.tfrs_listwise_loss_bwd(kind, y, s, n, l, sc, out, None)
  ndcg = lambda y, s, n, l, topn, a, b: lib.tfrs_listwise_ndcg(y, s, n, l, topn, a, b, None)
  bad = [fwd(0, None, p, 2, 5, p), fwd(0, p, None, 2, 5, p), fwd(0, p, p, 2, 5, None),
         fwd(0, p, p, 2, 0, p), fwd(0, p, p, 2, 1025, p), fwd(4, p, p, 2, 5, p), fwd(-1, p, p, 2, 5, p),
         fwd(0, p, p, -1, 5, p), fwd(0, p, p, 2 ** 31 // 1024, 1024, p),
         bwd(1, p, p, 2, 5, None, p), bwd(1, p, p, 2, 5, p, None), bwd(1, p, p, 2, 0, p, p),
         bwd(1, p, p, 2, 1025, p, p), bwd(7, p, p, 2, 5, p, p),
         ndcg(p, p, 2, 5, -1, p, p), ndcg(p, p, 2, 0, 0, p, p), ndcg(p, p, 2, 1025, 0, p, p),
         ndcg(None, p, 2, 5, 0, p, p), ndcg(p, p, 2, 5, 0, p, None)]
  assert bad == [_lib.TFRS_EINVAL] * len(bad)
  assert fwd(9, p, p, 2, 5, p) == _lib.TFRS_EINVAL and "listwise_loss_fwd" in _lib.last_error()
  assert ndcg(p, p, 2, 5, -1, p, p) == _lib.TFRS_EINVAL and "topn" in _lib.last_error()
  # no lists: OK, and nothing is launched (there is no device here to launch on)
  assert fwd(0, None, None, 0, 5, None) == _lib.TFRS_OK
  assert bwd(3, None, None, 0, 5, None, None) == _lib.TFRS_OK
  assert ndcg(None, None, 0, 5, 3, None, None) == _lib.TFRS_OK
