"""Lambda weights without a GPU: the float64 restatement (tests/lambda_weight_restatement.py) against the LambdaRank
identity (a pair's weight is the change of NDCG when the two items swap ranks -- computed with the NDCG restatement of
tests/listwise_restatement.py, which shares nothing with the weight code), closed forms, finite differences at fixed
ranks, hand-computed smooth terms and the zero-weight cases; the row-vectorised reference the GPU tests use against the
explicit loops; and the host-side validation of the product classes and of the two C entries (which reject bad
arguments before any device call)."""

import math

import numpy as np
import pytest
import torch

from tests import lambda_weight_restatement as lam
from tests import listwise_restatement as lw

KINDS = (lam.PAIRWISE_LOGISTIC, lam.PAIRWISE_HINGE)
D0 = lam.d0


# ---- the LambdaRank identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 7, 12])
def test_ndcg_weight_is_the_ndcg_change_of_a_swap(n):
  """Distinct scores, mu = 0, normalised: w_ij = |NDCG(s with s_i, s_j swapped) - NDCG(s)| for topn in {None, 1, 3, n}."""
  rng = np.random.RandomState(20 + n)
  for trial in range(4):
    y = rng.randint(0, 5, size=n + 2).astype(np.float64)
    y[0] = max(y[0], 1.0)
    y[rng.randint(1, n + 2, size=2)] = -1.0                  # one or two pads anywhere
    s = rng.permutation(n + 2) * 0.37 - 1.0                  # distinct
    for topn in (None, 1, 3, n):
      base = lw.list_ndcg(y, s, topn)[0]
      ws = lam.pair_weights(y, s, lam.Config(topn, True, 0.0))
      assert len(ws) == sum(1 for i in range(n + 2) for j in range(n + 2) if y[j] >= 0 and y[i] > y[j])
      for (i, j), w in ws.items():
        sw = s.copy()
        sw[i], sw[j] = s[j], s[i]
        assert w == pytest.approx(abs(lw.list_ndcg(y, sw, topn)[0] - base), rel=1e-12, abs=1e-15), (topn, i, j)


def test_dcg_weight_is_the_dcg_change_of_a_swap():
  y = [3.0, 0.0, -1.0, 1.0, 2.0]
  s = [0.1, 0.9, 5.0, 0.5, -0.3]
  for topn in (None, 2):
    ws = lam.pair_weights(y, s, lam.Config(topn, False, 0.0))
    for (i, j), w in ws.items():
      sw = list(s)
      sw[i], sw[j] = s[j], s[i]
      a = lw._dcg(lw.score_order(y, s), y, topn).value
      b = lw._dcg(lw.score_order(y, sw), y, topn).value
      assert w == pytest.approx(abs(a - b), rel=1e-13, abs=1e-15)


# ---- closed forms ----------------------------------------------------------------------------------------------------
def test_two_items_closed_forms():
  # y = (1, 0): one pair, ranks {1, 2} whichever way the scores go; DCG weight 1 * (1 - 1 / log2 3), NDCG the same
  # (IDCG = 1); both kinds, both score orders
  w = 1.0 - 1.0 / math.log2(3.0)
  for s in ([0.3, -1.2], [-0.5, 0.25]):
    x = s[0] - s[1]
    for cfg in (lam.Config(None, False, 0.0), lam.Config(None, True, 0.0), lam.Config(2, True, 0.0)):
      loss, grad = lam.list_loss(lam.PAIRWISE_LOGISTIC, [1.0, 0.0], s, cfg)
      assert loss.value == pytest.approx(w * math.log1p(math.exp(-x)), rel=1e-14)
      sig = w / (1.0 + math.exp(x))
      np.testing.assert_allclose(grad.value, [-sig, sig], rtol=1e-13)
      loss, grad = lam.list_loss(lam.PAIRWISE_HINGE, [1.0, 0.0], s, cfg)
      assert loss.value == pytest.approx(w * max(0.0, 1.0 - x), rel=1e-14)           # (x = 1.5 meets the margin)
      np.testing.assert_allclose(grad.value, [-w, w] if x < 1.0 else [0.0, 0.0], rtol=1e-14)
  # labels (2, 0): the gain difference is 3, and normalised it is 1 again (IDCG = 3)
  assert lam.pair_weights([2.0, 0.0], [0.0, 1.0], lam.Config(None, False, 0.0))[(0, 1)] == pytest.approx(3.0 * w, rel=1e-15)
  assert lam.pair_weights([2.0, 0.0], [0.0, 1.0], lam.Config(None, True, 0.0))[(0, 1)] == pytest.approx(w, rel=1e-15)
  # topn = 1: the second rank's discount is cut: v = 1
  assert lam.pair_weights([2.0, 0.0], [0.0, 1.0], lam.Config(1, False, 0.0))[(0, 1)] == pytest.approx(3.0, rel=1e-15)


def test_three_items_closed_form():
  # labels (2, 1, 0), scores rank the items 2, 0, 1 -> ranks r = (2, 3, 1); gains (3, 1, 0); IDCG = 3 + 1 / log2 3
  y, s = [2.0, 1.0, 0.0], [0.5, -1.0, 2.0]
  assert lam.ranks(y, s) == {2: 1, 0: 2, 1: 3}
  d = {1: 1.0, 2: 1.0 / math.log2(3.0), 3: 0.5}
  want = {(0, 1): 2.0 * (d[2] - d[3]), (0, 2): 3.0 * (d[1] - d[2]), (1, 2): 1.0 * (d[1] - d[3])}
  got = lam.pair_weights(y, s)
  assert set(got) == set(want)
  for k in want:
    assert got[k] == pytest.approx(want[k], rel=1e-14)
  idcg = 3.0 + 1.0 / math.log2(3.0)
  got = lam.pair_weights(y, s, lam.Config(None, True, 0.0))
  for k in want:
    assert got[k] == pytest.approx(want[k] / idcg, rel=1e-14)
  # hinge: x = (1.5, -1.5, -3): every pair active
  loss, grad = lam.list_loss(lam.PAIRWISE_HINGE, y, s)
  assert loss.value == pytest.approx(want[(0, 1)] * 0.0 + want[(0, 2)] * 2.5 + want[(1, 2)] * 4.0, rel=1e-14)
  np.testing.assert_allclose(grad.value, [-want[(0, 2)], -want[(1, 2)], want[(0, 2)] + want[(1, 2)]], rtol=1e-13)
  # topn = 2, normalised: IDCG@2 is the same; rank 3 is cut: D = (d2, 0, 1)
  got = lam.pair_weights(y, s, lam.Config(2, True, 0.0))
  assert got[(0, 1)] == pytest.approx(2.0 * d[2] / idcg, rel=1e-14)
  assert got[(1, 2)] == pytest.approx(1.0 / idcg, rel=1e-14)


# ---- smooth fractions by hand ----------------------------------------------------------------------------------------
def test_smooth_fraction_by_hand():
  y, s = [2.0, 1.0, 0.0], [0.5, -1.0, 2.0]                   # ranks (2, 3, 1) as above
  d = {1: 1.0, 2: 1.0 / math.log2(3.0), 3: 0.5, 4: 1.0 / math.log2(5.0)}
  u = {1: d[1] - d[2], 2: d[2] - d[3], 3: d[3] - d[4]}       # u(delta) = D0(delta) - D0(delta + 1)
  assert u[1] == pytest.approx(1.0 - 0.6309297535714574, rel=1e-15)
  v = {(0, 1): d[2] - d[3], (0, 2): d[1] - d[2], (1, 2): d[1] - d[3]}
  delta = {(0, 1): 1, (0, 2): 1, (1, 2): 2}
  dg = {(0, 1): 2.0, (0, 2): 3.0, (1, 2): 1.0}
  for mu in (1.0, 0.25):
    got = lam.pair_weights(y, s, lam.Config(None, False, mu))
    for k in v:
      assert got[k] == pytest.approx(dg[k] * ((1.0 - mu) * v[k] + mu * u[delta[k]]), rel=1e-14), (mu, k)
  # mu = 1 does not look at the discounts of the ranks at all, but the cut still applies: topn = 1 kills (0, 1) only
  got = lam.pair_weights(y, s, lam.Config(1, False, 1.0))
  assert got[(0, 1)] == 0.0 and got[(0, 2)] == pytest.approx(3.0 * u[1]) and got[(1, 2)] == pytest.approx(u[2])


# ---- zero weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_zero_weight_cases(kind):
  s = [0.3, -1.0, 0.7, 2.0]
  for cfg in (lam.Config(), lam.Config(None, True, 0.0), lam.Config(2, True, 0.25), lam.Config(None, False, 1.0)):
    for y in ([2.0, 2.0, -1.0, 2.0], [0.0, 0.0, 0.0, -1.0], [-1.0] * 4, [-1.0, 3.0, -1.0, -1.0]):
      loss, grad = lam.list_loss(kind, y, s, cfg)           # P empty (equal labels; IDCG = 0; n = 0; n = 1)
      assert loss.value == 0.0 and not grad.value.any() and loss.bound == 0.0
  # both items beyond topn: labels (3, 0, 2, 1), ranks by score (3, 4, 2, 1); topn = 2 -> the pair (0, 1) weighs 0 ...
  y = [3.0, 0.0, 2.0, 1.0]
  assert lam.ranks(y, s) == {3: 1, 2: 2, 0: 3, 1: 4}
  for mu in (0.0, 0.25, 1.0):
    for normalized in (False, True):
      ws = lam.pair_weights(y, s, lam.Config(2, normalized, mu))
      assert ws[(0, 1)] == 0.0
      assert all(w > 0.0 for k, w in ws.items() if k != (0, 1))
  # ... so the loss does not feel the scores of that pair's far side: moving item 1 (rank 4, paired with everything)
  # changes the loss only through its pairs with the items inside the cut
  cfg = lam.Config(2, True, 0.25)
  _, grad = lam.list_loss(kind, y, s, cfg)
  ws = lam.pair_weights(y, s, cfg)
  want = -sum(ws[(i, 1)] * lw._dphi(kind, s[i] - s[1]) for i in (2, 3))
  assert grad.value[1] == pytest.approx(want, rel=1e-14)


# ---- gradients: finite differences at fixed ranks --------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_match_finite_differences_at_fixed_ranks(kind):
  """Scores on a grid of step 0.4 (+- 0.05 of jitter, so no hinge pair sits on its kink): the gaps are far above the
  step h = 1e-5, the ranks and with them the weights -- constants by contract -- do not move."""
  rng = np.random.RandomState(9 + kind)
  for L in (2, 5, 11):
    for cfg in (lam.Config(), lam.Config(None, True, 0.0), lam.Config(3, True, 0.25), lam.Config(None, False, 1.0)):
      y = rng.randint(-1, 5, size=L).astype(np.float64)
      s = rng.permutation(L) * 0.4 - 1.0 + rng.uniform(-0.05, 0.05, size=L)
      assert all(abs(1.0 - (s[i] - s[j])) > 0.05 for i in range(L) for j in range(L) if i != j)
      _, grad = lam.list_loss(kind, y, s, cfg)
      h = 1e-5
      for k in range(L):
        sp, sm = s.copy(), s.copy()
        sp[k] += h
        sm[k] -= h
        assert lam.ranks(y, sp) == lam.ranks(y, sm) == lam.ranks(y, s)
        fd = (lam.list_loss(kind, y, sp, cfg)[0].value - lam.list_loss(kind, y, sm, cfg)[0].value) / (2.0 * h)
        assert grad.value[k] == pytest.approx(fd, rel=1e-6, abs=1e-8), (kind, L, cfg, k)
        if y[k] < 0:
          assert grad.value[k] == 0.0


# ---- the unweighted loss is the weight-one special case; the fast reference is the slow one -----------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_row_vectorised_reference_equals_the_explicit_loops(kind):
  for B, L in ((3, 1), (4, 2), (5, 9), (4, 33)):
    y, s = lw.make_labels(B, L, 60 + L), lw.make_scores(B, L, 60 + L)
    if L >= 9:
      s[0, 3] = s[0, 1]                                     # a tie
      y[1] = np.where(y[1] >= 0, 0.0, -1.0)                 # IDCG = 0
    for cfg in lam.configs(L).values():
      bl, bg = lam.batch_loss(kind, y, s, cfg)
      for b in range(B):
        ll, lg = lam.list_loss(kind, y[b], s[b], cfg)
        for got, want in ((bl.value[b], ll.value), (bl.yard[b], ll.yard), (bl.u[b], ll.u), (bl.bound[b], ll.bound)):
          assert got == pytest.approx(float(want), rel=1e-11, abs=1e-300)
        assert bl.n[b] == ll.n
        np.testing.assert_allclose(bg.value[b], lg.value, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(bg.bound[b], lg.bound, rtol=1e-11, atol=1e-300)
        np.testing.assert_array_equal(bg.n[b], lg.n)


def test_bound_dominates_float32_evaluation_of_the_same_formulas():
  """The derived bound against a plain numpy float32 evaluation (one more, independent summation order): it must hold
  there too, with room, or the derivation forgot a term."""
  f = np.float32
  for L, cfg in ((9, lam.Config(None, True, 0.0)), (33, lam.Config(3, True, 0.25)), (33, lam.Config(None, False, 1.0))):
    y, s = lw.make_labels(4, L, 70 + L), lw.make_scores(4, L, 70 + L)
    ref, _ = lam.batch_loss(lam.PAIRWISE_HINGE, y, s, cfg)
    for b in range(4):
      wt = lam.Weights([float(v) for v in y[b]], [float(v) for v in s[b]], cfg)
      idcg = f(0.0)
      if cfg.normalized:
        pi = lw.label_order(list(y[b]))
        k = len(pi) if cfg.topn is None else min(len(pi), cfg.topn)
        for r in range(1, k + 1):
          idcg = f(idcg + f(f(np.exp2(f(y[b, pi[r - 1]]))) - f(1.0)) / f(np.log2(f(r + 1))))
      tot = f(0.0)
      for i in wt.rank:
        for j in wt.rank:
          if y[b, i] > y[b, j]:
            g = [f(np.exp2(f(y[b, t]))) - f(1.0) for t in (i, j)]
            if cfg.normalized:
              g = [f(t / idcg) if idcg > 0 else f(0.0) for t in g]
            dd = [f(1.0) / f(np.log2(f(wt.rank[t] + 1))) if cfg.topn is None or wt.rank[t] <= cfg.topn else f(0.0)
                  for t in (i, j)]
            dl = abs(wt.rank[i] - wt.rank[j])
            u = abs(f(1.0) / f(np.log2(f(dl + 1))) - f(1.0) / f(np.log2(f(dl + 2))))
            c = f(f(f(1.0) - f(cfg.mu)) * abs(f(dd[0] - dd[1]))) + f(f(cfg.mu) * u)
            if cfg.topn is not None and min(wt.rank[i], wt.rank[j]) > cfg.topn:
              c = f(0.0)
            w = f(abs(f(g[0] - g[1])) * f(c))
            tot = f(tot + f(w * max(f(0.0), f(f(1.0) - f(s[b, i] - s[b, j])))))
      assert abs(float(tot) - ref.value[b]) <= ref.bound[b] + lam.FLOOR, (L, cfg, b)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_constructors_and_arguments_are_validated():
  from recommenders_amd import losses
  for cls in (losses.DCGLambdaWeight, losses.NDCGLambdaWeight):
    for bad in (0, -3, 2.5, "3", True):
      with pytest.raises(ValueError, match="topn"):
        cls(topn=bad)
    for bad in (-0.01, 1.5, float("nan"), "x", None):
      with pytest.raises(ValueError, match="smooth_fraction"):
        cls(smooth_fraction=bad)
    w = cls(topn=5, smooth_fraction=0.25)
    assert w.topn == 5 and w.smooth_fraction == 0.25
    assert cls().topn is None and cls().smooth_fraction == 0.0
  assert losses.NDCGLambdaWeight().normalized is True and isinstance(losses.NDCGLambdaWeight(), losses.DCGLambdaWeight)
  assert losses.DCGLambdaWeight().normalized is False and losses.DCGLambdaWeight(normalized=True).normalized is True
  with pytest.raises(TypeError):
    losses.NDCGLambdaWeight(normalized=False)
  for cls in (losses.PairwiseLogisticLoss, losses.PairwiseHingeLoss):
    assert cls().lambda_weight is None and cls(lambda_weight=None).lambda_weight is None
    w = losses.NDCGLambdaWeight(topn=3)
    assert cls(lambda_weight=w).lambda_weight is w
    assert cls("sum", "mine", w).lambda_weight is w          # after `name`: TF-Ranking's argument order
    for bad in (1.0, "ndcg", losses.NDCGLambdaWeight, object()):
      with pytest.raises(ValueError, match="lambda_weight"):
        cls(lambda_weight=bad)
    loss = cls(lambda_weight=w)
    y, s = torch.zeros(4, 5), torch.zeros(4, 5)
    with pytest.raises(ValueError, match="per list"):
      loss(y, s, sample_weight=torch.ones(4, 5))
    with pytest.raises(ValueError, match="MAX_LIST_LEN"):
      loss(torch.zeros(2, 1025), torch.zeros(2, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      loss(y, s)
  for cls in (losses.SoftmaxLoss, losses.ListMLELoss):
    with pytest.raises(TypeError):
      cls(lambda_weight=losses.NDCGLambdaWeight())


def test_c_entries_reject_bad_arguments_before_any_device_call():
  import ctypes
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  lib = _lib.load()
  p = ctypes.c_void_p(256)       # never dereferenced: every call below returns before a launch
  fwd = lambda kind, y, s, n, l, topn, norm, mu, out: lib.tfrs_listwise_lambda_fwd(kind, y, s, n, l, topn, norm, mu, out, None)
  bwd = lambda kind, y, s, n, l, topn, norm, mu, sc, out: lib.tfrs_listwise_lambda_bwd(kind, y, s, n, l, topn, norm, mu, sc,
                                                                                       out, None)
  nan = float("nan")
  bad = {
      "fwd kind 0": fwd(0, p, p, 2, 5, 0, 1, 0.0, p), "fwd kind 3": fwd(3, p, p, 2, 5, 0, 1, 0.0, p),
      "fwd kind 4": fwd(4, p, p, 2, 5, 0, 1, 0.0, p), "fwd kind -1": fwd(-1, p, p, 2, 5, 0, 1, 0.0, p),
      "fwd topn": fwd(1, p, p, 2, 5, -1, 1, 0.0, p), "fwd mu < 0": fwd(1, p, p, 2, 5, 0, 1, -0.5, p),
      "fwd mu > 1": fwd(1, p, p, 2, 5, 0, 1, 1.5, p), "fwd mu nan": fwd(2, p, p, 2, 5, 0, 0, nan, p),
      "fwd len 0": fwd(1, p, p, 2, 0, 0, 1, 0.0, p), "fwd len 1025": fwd(1, p, p, 2, 1025, 0, 1, 0.0, p),
      "fwd 2^31": fwd(1, p, p, 2 ** 31 // 1024, 1024, 0, 1, 0.0, p), "fwd nlists < 0": fwd(1, p, p, -1, 5, 0, 1, 0.0, p),
      "fwd NULL labels": fwd(1, None, p, 2, 5, 0, 1, 0.0, p), "fwd NULL scores": fwd(1, p, None, 2, 5, 0, 1, 0.0, p),
      "fwd NULL loss": fwd(2, p, p, 2, 5, 0, 1, 0.25, None),
      "bwd kind 0": bwd(0, p, p, 2, 5, 0, 1, 0.0, p, p), "bwd kind 3": bwd(3, p, p, 2, 5, 0, 1, 0.0, p, p),
      "bwd kind 4": bwd(4, p, p, 2, 5, 0, 1, 0.0, p, p), "bwd topn": bwd(2, p, p, 2, 5, -7, 0, 0.0, p, p),
      "bwd mu < 0": bwd(1, p, p, 2, 5, 0, 1, -1e-3, p, p), "bwd mu > 1": bwd(1, p, p, 2, 5, 0, 1, 1.001, p, p),
      "bwd mu nan": bwd(1, p, p, 2, 5, 0, 1, nan, p, p), "bwd len 0": bwd(1, p, p, 2, 0, 0, 1, 0.0, p, p),
      "bwd len 1025": bwd(1, p, p, 2, 1025, 0, 1, 0.0, p, p),
      "bwd 2^31": bwd(1, p, p, 2 ** 31 // 1024, 1024, 0, 1, 0.0, p, p),
      "bwd NULL labels": bwd(1, None, p, 2, 5, 0, 1, 0.0, p, p), "bwd NULL scores": bwd(1, p, None, 2, 5, 0, 1, 0.0, p, p),
      "bwd NULL scale": bwd(1, p, p, 2, 5, 0, 1, 1.0, None, p), "bwd NULL dscores": bwd(2, p, p, 2, 5, 0, 1, 0.0, p, None),
  }
  assert {k: v for k, v in bad.items() if v != _lib.TFRS_EINVAL} == {}
  assert fwd(0, p, p, 2, 5, 0, 1, 0.0, p) == _lib.TFRS_EINVAL and "listwise_lambda_fwd" in _lib.last_error()
  assert bwd(1, p, p, 2, 5, 0, 1, 2.0, p, p) == _lib.TFRS_EINVAL and "smooth_fraction" in _lib.last_error()
  # no lists: OK, and nothing is launched (there is no device here to launch on)
  assert fwd(1, None, None, 0, 5, 3, 1, 0.25, None) == _lib.TFRS_OK
  assert bwd(2, None, None, 0, 5, 0, 0, 1.0, None, None) == _lib.TFRS_OK
  # the unweighted entries still know four kinds only
  assert lib.tfrs_listwise_loss_fwd(4, p, p, 2, 5, p, None) == _lib.TFRS_EINVAL
