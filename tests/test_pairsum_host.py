"""The pair-sum losses (ApproxNDCG, ApproxMRR, UniqueSoftmax) without a GPU: the float64 restatement
(tests/pairsum_restatement.py) against closed forms, central differences, torch float64 autograd of the explicit
[L, L] composition, its identities and its hard limit; the exactness condition that makes the GPU test's ApproxMRR
bit-equality legitimate; and the host-side validation of the product classes and of the C entries (which reject bad
arguments before any device call)."""

import math
import os

import numpy as np
import pytest
import torch

from tests import listwise_restatement as lw
from tests import pairsum_restatement as ps

ALL_KINDS = (ps.APPROX_NDCG, ps.APPROX_MRR, ps.UNIQUE_SOFTMAX)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sigma(x):
  return 1.0 / (1.0 + math.exp(-x))


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.1, 1.0, 3.0])
def test_one_valid_item(temperature):
  """r = 1: ApproxNDCG is -G / (G log2 2) = -1 for a positive label, ApproxMRR -y / (y 1) = -1, UniqueSoftmax
  G (log e^t - t) = 0; nothing depends on the score, so every gradient is 0."""
  for y, s in (([3.0], [0.7]), ([-1.0, 2.0, -1.0], [9.0, -1.3, 5.0])):
    for kind, want in ((ps.APPROX_NDCG, -1.0), (ps.APPROX_MRR, -1.0), (ps.UNIQUE_SOFTMAX, 0.0)):
      loss, grad = ps.list_loss(kind, y, s, temperature)
      assert loss.value == pytest.approx(want, abs=1e-15)
      assert not grad.value.any()
  for kind in (ps.APPROX_NDCG, ps.APPROX_MRR):      # the one valid label is 0: no loss
    loss, grad = ps.list_loss(kind, [0.0, -1.0], [0.3, 0.1], temperature)
    assert loss.value == 0.0 and not grad.value.any()


@pytest.mark.parametrize("a,b,temperature", [(0.3, -1.2, 1.0), (-2.0, 1.5, 0.5), (0.0, 0.0, 0.1), (0.25, 0.5, 0.125)])
def test_two_items_by_hand(a, b, temperature):
  """y = (2, 0), s = (a, b), alpha = float32(1 / temperature), p = sigma(alpha (b - a)):
  r = (1 + p, 2 - p).  IDCG = 3; ApproxNDCG = -(3 / log2(2 + p)) / 3; ApproxMRR = -(2 / (1 + p)) / 2;
  UniqueSoftmax = 3 (log(e^{alpha a} + e^{alpha b}) - alpha a) = 3 log(1 + e^{alpha (b - a)})."""
  alpha = ps.alpha_of(temperature)
  p = _sigma(alpha * (b - a))
  dp = p * (1.0 - p) * alpha                          # dp/db = -dp/da
  loss, grad = ps.list_loss(ps.APPROX_NDCG, [2.0, 0.0], [a, b], temperature)
  assert loss.value == pytest.approx(-1.0 / math.log2(2.0 + p), rel=1e-14)
  dl = dp / (math.log2(2.0 + p) ** 2 * (2.0 + p) * math.log(2.0))      # dl/db
  np.testing.assert_allclose(grad.value, [-dl, dl], rtol=1e-12)
  loss, grad = ps.list_loss(ps.APPROX_MRR, [2.0, 0.0], [a, b], temperature)
  assert loss.value == pytest.approx(-1.0 / (1.0 + p), rel=1e-14)
  np.testing.assert_allclose(grad.value, [-dp / (1.0 + p) ** 2, dp / (1.0 + p) ** 2], rtol=1e-12)
  loss, grad = ps.list_loss(ps.UNIQUE_SOFTMAX, [2.0, 0.0], [a, b], temperature)
  x = alpha * (b - a)
  assert loss.value == pytest.approx(3.0 * (max(x, 0.0) + math.log1p(math.exp(-abs(x)))), rel=1e-13)
  np.testing.assert_allclose(grad.value, [-3.0 * alpha * _sigma(x), 3.0 * alpha * _sigma(x)], rtol=1e-12)


# ---- gradients -------------------------------------------------------------------------------------------------------
def _inputs(L, seed):
  rng = np.random.RandomState(seed)
  y = rng.randint(-1, 5, size=L).astype(np.float64)
  return y, rng.randn(L) * 2.0


@pytest.mark.parametrize("temperature", [0.1, 1.0])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_gradients_match_central_differences(kind, temperature):
  for L in (1, 2, 5, 11):
    y, s = _inputs(L, 5 + kind + L)
    _, grad = ps.list_loss(kind, y, s, temperature)
    h = 1e-6
    for k in range(L):
      sp, sm = s.copy(), s.copy()
      sp[k] += h
      sm[k] -= h
      fd = (ps.list_loss(kind, y, sp, temperature)[0].value - ps.list_loss(kind, y, sm, temperature)[0].value) / (2 * h)
      assert grad.value[k] == pytest.approx(fd, rel=2e-6, abs=1e-7), (kind, L, k)
      if y[k] < 0:
        assert grad.value[k] == 0.0


def explicit_composition(kind, y, s, alpha):
  """The losses as torch ops on the explicit [L, L] pair matrices of one list (any float dtype, any device)."""
  valid = y >= 0
  pair = valid[:, None] & valid[None, :]
  off = pair & ~torch.eye(len(y), dtype=torch.bool, device=y.device)
  gain = torch.where(valid, torch.exp2(y) - 1.0, torch.zeros_like(y))
  if kind == ps.UNIQUE_SOFTMAX:
    t = alpha * s
    M = (pair & (y[None, :] < y[:, None])) | torch.eye(len(y), dtype=torch.bool, device=y.device)
    lse = torch.logsumexp(torch.where(M, t[None, :].expand(len(y), -1), torch.full_like(t, -float("inf"))[None, :]), dim=1)
    return torch.where(valid, gain * (lse - t), torch.zeros_like(t)).sum()
  sig = torch.sigmoid(alpha * (s[None, :] - s[:, None]))
  r = 1.0 + torch.where(off, sig, torch.zeros_like(sig)).sum(dim=1)
  if kind == ps.APPROX_NDCG:
    n = int(valid.sum())
    ideal = torch.sort(torch.where(valid, gain, torch.full_like(gain, -1.0)), descending=True).values[:n]
    idcg = (ideal / torch.log2(torch.arange(n, dtype=y.dtype, device=y.device) + 2.0)).sum()
    if not idcg > 0:
      return 0.0 * s.sum()
    return -(gain / torch.log2(1.0 + r)).sum() / idcg
  ysum = torch.where(valid, y, torch.zeros_like(y)).sum()
  if not ysum > 0:
    return 0.0 * s.sum()
  return -(torch.where(valid, y, torch.zeros_like(y)) / r).sum() / ysum


@pytest.mark.parametrize("temperature", [0.1, 1.0])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_values_and_gradients_match_torch_autograd_of_the_explicit_composition(kind, temperature):
  for L in (1, 2, 5, 11, 40):
    y, s = _inputs(L, 31 + kind + L)
    loss, grad = ps.list_loss(kind, y, s, temperature)
    st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    out = explicit_composition(kind, torch.tensor(y, dtype=torch.float64), st, ps.alpha_of(temperature))
    out.backward()
    assert loss.value == pytest.approx(float(out.detach()), rel=1e-12, abs=1e-13)
    np.testing.assert_allclose(grad.value, st.grad.numpy(), rtol=1e-10, atol=1e-12)


# ---- identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.1, 1.0])
def test_soft_ranks_sum_to_n_n_plus_1_over_2_and_gradients_sum_to_zero(temperature):
  """sigma(x) + sigma(-x) = 1 for every pair, so sum_V r_i = n + n (n - 1) / 2; a common shift of the scores changes
  no loss, so every gradient sums to 0."""
  for L in (2, 5, 11, 40):
    y, s = _inputs(L, 61 + L)
    V = y >= 0
    n = int(V.sum())
    r = ps.soft_ranks(s[V], ps.alpha_of(temperature))[0]
    assert r.sum() == pytest.approx(n * (n + 1) / 2.0, rel=1e-13)
    for kind in ALL_KINDS:
      _, grad = ps.list_loss(kind, y, s, temperature)
      assert abs(grad.value.sum()) <= 1e-12 * max(np.abs(grad.value).sum(), 1.0)


# ---- the hard limit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 11, 40])
def test_small_temperature_gives_the_metric(L):
  """Distinct scores on a 0.5 grid, temperature 0.01: a pair contributes at most e^-50 to a rank, n^2 e^-50 < 1e-15 in
  all, so the soft ranks are the ranks to 1e-15 and ApproxNDCG = -NDCG, ApproxMRR = -sum y_i / rank_i / Y to 1e-9."""
  rng = np.random.RandomState(70 + L)
  y = rng.randint(-1, 5, size=L).astype(np.float64)
  y[0] = 3.0
  s = rng.permutation(L) * 0.5 - 3.0
  ndcg, counted, _ = lw.list_ndcg(y, s)
  assert counted == 1.0
  assert ps.list_loss(ps.APPROX_NDCG, y, s, 0.01)[0].value == pytest.approx(-ndcg, abs=1e-9)
  order = lw.score_order(list(y), list(s))
  want = -sum(y[i] / (rank + 1.0) for rank, i in enumerate(order)) / sum(y[i] for i in order)
  assert ps.list_loss(ps.APPROX_MRR, y, s, 0.01)[0].value == pytest.approx(want, abs=1e-9)


# ---- padding and degenerate lists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_pads_and_lists_without_a_loss(kind):
  y, s = [2.0, 0.0, 3.0, 1.0, 1.0], [0.3, -1.0, 0.7, 2.0, -0.4]
  base_loss, base_grad = ps.list_loss(kind, y, s, 0.5)
  for at in range(len(y) + 1):
    loss, grad = ps.list_loss(kind, y[:at] + [-1.0] + y[at:], s[:at] + [1e30] + s[at:], 0.5)
    assert loss.value == pytest.approx(base_loss.value, rel=1e-14)
    np.testing.assert_allclose(np.delete(grad.value, at), base_grad.value, rtol=1e-13)
    assert grad.value[at] == 0.0
  loss, grad = ps.list_loss(kind, [-1.0, -1.0, -1.0], [1.0, 2.0, 3.0], 0.5)
  assert loss.value == 0.0 and not grad.value.any() and loss.bound == 0.0
  if kind != ps.UNIQUE_SOFTMAX:
    loss, grad = ps.list_loss(kind, [0.0, 0.0, -1.0, 0.0], [1.0, 2.0, 9.0, 3.0], 0.5)
    assert loss.value == 0.0 and not grad.value.any()


# ---- the exact cases of the GPU ApproxMRR test -----------------------------------------------------------------------
@pytest.mark.parametrize("temperature", ps.MRR_EXACT_TEMPERATURES)
@pytest.mark.parametrize("n", ps.MRR_EXACT_N)
def test_approx_mrr_exact_inputs_are_exact(n, temperature):
  """Every input set the GPU test compares bit for bit: all valid scores of a list equal, labels in {0, 1} with one or
  two ones, n + 1 a power of two, power-of-two temperature and weights; every partial sum of every order is a float32
  (tests/pairsum_restatement.py: mrr_exact_ok says why), r = (n + 1) / 2 and the loss is -2 / (n + 1)."""
  y, s, w = ps.mrr_exact_inputs(n)
  assert y.shape == (4, n + 1) and (y == -1.0).sum() == 4 and set(np.unique(y)) <= {-1.0, 0.0, 1.0}
  assert sorted(int((row == 1.0).sum()) for row in y) == ([1, 1, 1, 1] if n < 2 else [1, 1, 2, 2])
  assert ps.mrr_exact_ok(y, s, w, temperature)
  loss, grad = ps.batch_loss(ps.APPROX_MRR, y, s, temperature)
  np.testing.assert_array_equal(loss.value, -2.0 / (n + 1))
  assert np.array_equal(grad.value.astype(np.float32).astype(np.float64), grad.value)
  for b in range(4):
    V = y[b] >= 0
    np.testing.assert_array_equal(ps.soft_ranks(s[b][V].astype(np.float64), ps.alpha_of(temperature))[0], (n + 1) / 2.0)


def test_approx_mrr_exact_condition_rejects_what_it_should():
  y, s, w = ps.mrr_exact_inputs(7)
  assert ps.mrr_exact_ok(y, s, w, 0.5)
  assert not ps.mrr_exact_ok(y, s, w, 0.3)                      # alpha no power of two
  s2 = s.copy()
  s2[0, 1] += 0.25                                              # a pair off x = 0
  assert not ps.mrr_exact_ok(y, s2, w, 0.5)
  assert not ps.mrr_exact_ok(y, s, w * 3.0, 0.5)                # weights no powers of two
  y2 = np.zeros((1, 6), dtype=np.float32)                       # n = 6: r = 3.5
  y2[0, 0] = 1.0
  assert not ps.mrr_exact_ok(y2, np.zeros((1, 6), dtype=np.float32), np.ones(1, dtype=np.float32), 0.5)
  assert not ps._exact_sum([1.0, 2.0 ** -24])                   # 2^24 + 1 steps
  assert ps._exact_sum([1.0] + [0.5] * 1022) and not ps._exact_sum([0.1])


# ---- the C surface and the host classes ------------------------------------------------------------------------------
def test_the_c_surface_is_declared():
  from recommenders_amd import _lib
  header = open(os.path.join(REPO, "include", "tfrs_hip.h")).read()
  for name in ("tfrs_listwise_pairsum_fwd", "tfrs_listwise_pairsum_bwd"):
    assert f"int {name}(" in header and name in _lib.SIGNATURES
  for name, value in (("APPROX_NDCG", 0), ("APPROX_MRR", 1), ("UNIQUE_SOFTMAX", 2)):
    assert f"#define TFRS_LISTWISE_{name} {value}\n" in header
  assert len(_lib.SIGNATURES["tfrs_listwise_pairsum_fwd"][1]) == 8
  assert len(_lib.SIGNATURES["tfrs_listwise_pairsum_bwd"][1]) == 9


def _classes():
  from recommenders_amd import losses
  return ((losses.ApproxNDCGLoss, "approx_ndcg_loss", 0.1), (losses.ApproxMRRLoss, "approx_mrr_loss", 0.1),
          (losses.UniqueSoftmaxLoss, "unique_softmax_loss", 1.0))


def test_constructors_and_shapes_are_validated_before_the_device():
  from recommenders_amd import losses
  y, s = torch.zeros(4, 5), torch.zeros(4, 5)
  for cls, name, temperature in _classes():
    loss = cls()
    assert loss.name == name and loss.temperature == temperature and loss.reduction == "sum_over_batch_size"
    assert cls(reduction="auto", temperature=2).temperature == 2.0
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-46, 1e-39, 1e39, None, "warm", True):
      with pytest.raises(ValueError, match="temperature"):
        cls(temperature=bad)
    with pytest.raises(TypeError, match="lambda_weight"):
      cls(lambda_weight=losses.NDCGLambdaWeight())
    with pytest.raises(ValueError, match="reduction"):
      cls(reduction="mean")
    with pytest.raises(ValueError, match="per list"):
      loss(y, s, sample_weight=torch.ones(4, 5))
    with pytest.raises(ValueError, match=r"\[batch, list\]"):
      loss(torch.zeros(5), torch.zeros(5))
    with pytest.raises(ValueError, match="MAX_LIST_LEN"):
      loss(torch.zeros(2, 1025), torch.zeros(2, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      loss(y, s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      loss(y, s, sample_weight=torch.ones(4, 1))


def test_c_entries_reject_bad_arguments_before_any_device_call():
  import ctypes
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  lib = _lib.load()
  p = ctypes.c_void_p(256)       # never dereferenced: every call below returns before a launch
  fwd = lambda kind, y, s, n, l, t, out: lib.tfrs_listwise_pairsum_fwd(kind, y, s, n, l, t, out, None)
  bwd = lambda kind, y, s, n, l, t, sc, out: lib.tfrs_listwise_pairsum_bwd(kind, y, s, n, l, t, sc, out, None)
  bad = [fwd(3, p, p, 2, 5, 1.0, p), fwd(-1, p, p, 2, 5, 1.0, p), bwd(3, p, p, 2, 5, 1.0, p, p),
         fwd(0, None, p, 2, 5, 1.0, p), fwd(1, p, None, 2, 5, 1.0, p), fwd(2, p, p, 2, 5, 1.0, None),
         bwd(0, p, p, 2, 5, 1.0, None, p), bwd(1, p, p, 2, 5, 1.0, p, None), bwd(2, None, p, 2, 5, 1.0, p, p),
         fwd(0, p, p, 2, 0, 1.0, p), fwd(0, p, p, 2, 1025, 1.0, p), bwd(2, p, p, 2, 0, 1.0, p, p),
         bwd(2, p, p, 2, 1025, 1.0, p, p), fwd(0, p, p, -1, 5, 1.0, p), fwd(0, p, p, 2 ** 31 // 1024, 1024, 1.0, p)]
  for t in (0.0, -1.0, float("nan"), float("inf"), 1e-46, 1e-39):
    bad += [fwd(0, p, p, 2, 5, t, p), bwd(2, p, p, 2, 5, t, p, p), fwd(1, None, None, 0, 5, t, None)]
  assert bad == [_lib.TFRS_EINVAL] * len(bad)
  assert fwd(9, p, p, 2, 5, 1.0, p) == _lib.TFRS_EINVAL and "listwise_pairsum_fwd" in _lib.last_error()
  assert bwd(0, p, p, 2, 5, 0.0, p, p) == _lib.TFRS_EINVAL and "temperature" in _lib.last_error()
  # no lists: OK, and nothing is launched (there is no device here to launch on)
  for kind in ALL_KINDS:
    assert fwd(kind, None, None, 0, 5, 0.1, None) == _lib.TFRS_OK
    assert bwd(kind, None, None, 0, 5, 0.1, None, None) == _lib.TFRS_OK
