"""``PairwiseLogisticLoss`` / ``PairwiseHingeLoss`` with ``lambda_weight=`` on the MI355X (the lambda kernels of
csrc/listwise.hip through losses.py) against the float64 restatement of tests/lambda_weight_restatement.py, under the
bound derived there (any summation order; ``float_gate`` with limit eps and the restatement's yardstick): value and
every gradient element.

Shapes: B in {1, 3, 67} x L in {1, 2, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130, 257, 1024} (B = 3 only at 1024): both sides
of every switch of the work mapping, one and several workgroups, the top of the envelope.  Configurations at every
shape: NDCGLambdaWeight(), DCGLambdaWeight(), topn in {1, 3, L, L + 5}, smooth_fraction in {0.25, 1}, and a cut
combined with a smooth fraction.  The reference of a shape is computed once per (kind, configuration) and shared."""

import functools

import numpy as np
import pytest
import torch

from tests import lambda_weight_restatement as lam
from tests import listwise_restatement as lw
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

GATE_FLOOR = lam.FLOOR / lam.EPS
KIND_NAMES = tuple(lam.KINDS)


def _loss_class(kind_name):
  from recommenders_amd import losses
  return {"pairwise_logistic": losses.PairwiseLogisticLoss, "pairwise_hinge": losses.PairwiseHingeLoss}[kind_name]


def _weight(cfg):
  from recommenders_amd import losses
  if cfg.normalized:
    return losses.NDCGLambdaWeight(topn=cfg.topn, smooth_fraction=cfg.mu)
  return losses.DCGLambdaWeight(topn=cfg.topn, smooth_fraction=cfg.mu)


def _cuda(a):
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(t):
  return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(kind_name, cfg, y, s, weight=None, reduction="none"):
  """(loss as returned, d (sum of the returned loss) / d scores) as numpy float32."""
  yt, st = _cuda(y), _cuda(s).requires_grad_(True)
  loss_fn = _loss_class(kind_name)(reduction=reduction, lambda_weight=_weight(cfg))
  out = loss_fn(yt, st, sample_weight=None if weight is None else _cuda(weight))
  out.sum().backward()
  return out.detach().cpu().numpy(), st.grad.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(B, L):
  seed = 500 * L + B
  return lw.make_labels(B, L, seed), lw.make_scores(B, L, seed)


@functools.lru_cache(maxsize=None)
def _reference(kind_name, config_name, B, L):
  y, s = _inputs(B, L)
  return lam.batch_loss(lam.KINDS[kind_name], y, s, lam.configs(L)[config_name])


def _gate(name, got, entry):
  return float_gate(name, got, entry.value, entry.gate, lam.EPS, floor=GATE_FLOOR)


def _padded_gradients_are_plus_zero(y, grad):
  pad = y < 0
  assert not grad[pad].any() and not np.signbit(grad[pad]).any()


# ---- 1. values and gradients against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("B,L", lam.SHAPES)
@pytest.mark.parametrize("config_name", lam.CONFIG_NAMES)
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_values_and_gradients_match_the_restatement(kind_name, config_name, B, L):
  y, s = _inputs(B, L)
  cfg = lam.configs(L)[config_name]
  ref_loss, ref_grad = _reference(kind_name, config_name, B, L)
  loss, grad = _run(kind_name, cfg, y, s)
  assert loss.shape == (B,) and grad.shape == (B, L) and loss.dtype == np.float32
  assert np.isfinite(loss).all() and np.isfinite(grad).all()
  el = _gate(f"lambda_weight.{kind_name}.loss", loss, ref_loss)
  eg = _gate(f"lambda_weight.{kind_name}.dscores", grad, ref_grad)
  print(f"{kind_name} {config_name} B={B} L={L}: loss error {el / lam.EPS:.3g}, gradient error {eg / lam.EPS:.3g} of the "
        f"bound (u up to {float(np.max(ref_loss.u)):.3g} / {float(np.max(ref_grad.u)):.3g})")
  _padded_gradients_are_plus_zero(y, grad)


# ---- 2. ties: ranks follow position -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 16, 33, 130, 1024])
def test_tied_scores_rank_by_position(L):
  """The ranks the kernel used, read from its output.  Labels: 1 at the FIRST valid item k of a list, 0 at every other
  valid item; DCG weight, mu = 0, hinge loss, reduction "sum"; scores on a coarse grid in [-0.25, 0.25] with s_k = 0.5
  (list 1: EVERY score equal, s_k included), so k has rank 1 (the top score, or the first position among equals),
  every pair (k, j) is active (|x| <= 0.75 < 1, phi' = -1) and
      d loss / d s_j = w_kj = |D0(1) - D0(r_j)| = 1 - D0(r_j):
  the gradient spells the rank of every other item.  1 - D0(r) is strictly increasing and its neighbouring values
  differ by more than 1.3e-5 at r <= 1024; the weight's error is at most (8 (1 + D0(r)) + w) eps <= 17 eps = 1e-6
  (tests/lambda_weight_restatement.py), so exactly one rank matches and it must be the restatement's."""
  from recommenders_amd import losses
  B = 4
  rng = np.random.RandomState(31 + L)
  y = np.zeros((B, L), dtype=np.float32)
  y[0, 2] = -1.0                                        # interior padding
  y[3, L - 2:] = -1.0                                   # trailing padding
  y[2, 0] = -1.0                                        # the key item is not position 0
  s = (rng.randint(-2, 3, size=(B, L)) * 0.125).astype(np.float32)
  s[2] = np.where(rng.rand(L) < 0.5, -0.25, 0.25)       # two values only
  key = [int(np.flatnonzero(y[b] >= 0)[0]) for b in range(B)]
  for b in range(B):
    y[b, key[b]] = 1.0
    s[b, key[b]] = 0.5
  s[1] = 0.125                                          # a whole list of equal scores
  yt, st = _cuda(y), _cuda(s).requires_grad_(True)
  loss = losses.PairwiseHingeLoss(reduction="sum", lambda_weight=losses.DCGLambdaWeight())(yt, st)
  loss.backward()
  grad = st.grad.cpu().numpy().astype(np.float64)
  table = np.array([1.0 - lam.d0(r) for r in range(1, L + 1)])      # table[r - 1] = w at rank r
  tol = (8.0 * (1.0 + (1.0 - table)) + table) * lam.EPS
  for b in range(B):
    want = lam.ranks([float(v) for v in y[b]], [float(v) for v in s[b]])
    assert want[key[b]] == 1
    got = {key[b]: 1}
    for j in want:
      if j != key[b]:
        hits = np.flatnonzero(np.abs(table - grad[b, j]) <= tol)
        assert len(hits) == 1, (L, b, j, grad[b, j], hits)
        got[j] = int(hits[0]) + 1
    assert got == want, (L, b)
    if b == 1:                                          # equal scores: ranks ascend with position
      valid = [j for j in range(L) if y[b, j] >= 0]
      assert [got[j] for j in valid] == list(range(1, len(valid) + 1))
  # and the full check under the bound, with gains that differ
  y2 = lw.make_labels(B, L, 37 + L)
  for cfg in (lam.Config(None, True, 0.0), lam.Config(3, True, 0.25)):
    for kind_name in KIND_NAMES:
      ref_loss, ref_grad = lam.batch_loss(lam.KINDS[kind_name], y2, s, cfg)
      got_loss, got_grad = _run(kind_name, cfg, y2, s)
      _gate(f"lambda_weight.{kind_name}.ties.loss", got_loss, ref_loss)
      _gate(f"lambda_weight.{kind_name}.ties.dscores", got_grad, ref_grad)


# ---- 3. padding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 257])
def test_interior_and_trailing_padding(L):
  """Removing the padded positions from a list (and padding the tail instead) changes no value beyond rounding of a
  different summation order: both layouts are held to the restatement of their own layout, and the restatements agree."""
  B = 3
  y, s = lw.make_labels(B, L, 83 + L), lw.make_scores(B, L, 83 + L)
  y[:, 1] = -1.0
  y[1, L // 2:] = -1.0
  yc, sc = np.full_like(y, -1.0), np.zeros_like(s)
  for b in range(B):
    keep = np.flatnonzero(y[b] >= 0)
    yc[b, :len(keep)], sc[b, :len(keep)] = y[b, keep], s[b, keep]
  for cfg in (lam.Config(None, True, 0.0), lam.Config(3, False, 0.25)):
    for kind_name in KIND_NAMES:
      ref_loss, ref_grad = lam.batch_loss(lam.KINDS[kind_name], y, s, cfg)
      ref_c, _ = lam.batch_loss(lam.KINDS[kind_name], yc, sc, cfg)
      np.testing.assert_allclose(ref_c.value, ref_loss.value, rtol=1e-12)
      for yy, ss, rl, rg in ((y, s, ref_loss, ref_grad), (yc, sc, ref_c, None)):
        loss, grad = _run(kind_name, cfg, yy, ss)
        _gate(f"lambda_weight.{kind_name}.padding.loss", loss, rl)
        if rg is not None:
          _gate(f"lambda_weight.{kind_name}.padding.dscores", grad, rg)
        _padded_gradients_are_plus_zero(yy, grad)


@pytest.mark.parametrize("L", [5, 64, 257])
def test_padded_scores_never_enter_the_arithmetic(L):
  B = 5
  y, s = lw.make_labels(B, L, 77 + L), lw.make_scores(B, L, 77 + L)
  y[0, L // 2] = -1.0
  pad = y < 0
  assert pad.any() and (~pad).any()
  cfgs = (lam.Config(None, True, 0.0), lam.Config(3, False, 0.25))
  base = {(k, c): _run(k, c, y, s) for k in KIND_NAMES for c in cfgs}
  for poison in (np.nan, np.inf, -np.inf, 1e30):
    sp = s.copy()
    sp[pad] = poison
    for (kind_name, cfg), (bl, bg) in base.items():
      loss, grad = _run(kind_name, cfg, y, sp)
      np.testing.assert_array_equal(loss.view(np.uint32), bl.view(np.uint32))
      np.testing.assert_array_equal(grad.view(np.uint32), bg.view(np.uint32))
      _padded_gradients_are_plus_zero(y, grad)


# ---- 4. degenerate lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 130])
def test_degenerate_lists_inside_a_normal_batch(L):
  B = 7
  y0, s0 = lw.make_labels(B, L, 41 + L), lw.make_scores(B, L, 41 + L)
  y0[:, 0] = np.maximum(y0[:, 0], 1.0)
  y, s = y0.copy(), s0.copy()
  y[1] = -1.0                                         # n = 0
  y[2] = -1.0
  y[2, L // 2] = 3.0                                  # n = 1
  y[3] = np.where(y0[3] >= 0, 2.0, -1.0)              # all labels equal
  y[5] = np.where(y0[5] >= 0, 0.0, -1.0)              # labels all zero: IDCG = 0
  for cfg in (lam.Config(None, True, 0.0), lam.Config(None, False, 0.0), lam.Config(3, True, 0.25)):
    for kind_name in KIND_NAMES:
      loss, grad = _run(kind_name, cfg, y, s)
      base_loss, base_grad = _run(kind_name, cfg, y0, s0)
      for b in (0, 4, 6):                             # the neighbours do not see the degenerate lists
        assert loss.view(np.uint32)[b] == base_loss.view(np.uint32)[b]
        np.testing.assert_array_equal(grad[b].view(np.uint32), base_grad[b].view(np.uint32))
      assert np.isfinite(loss).all() and np.isfinite(grad).all()
      for b in (1, 2, 3, 5):
        assert loss[b] == 0.0 and not grad[b].any() and not np.signbit(grad[b]).any(), (kind_name, cfg, b)
      assert loss[0] > 0.0
      ref_loss, ref_grad = lam.batch_loss(lam.KINDS[kind_name], y, s, cfg)
      _gate(f"lambda_weight.{kind_name}.degenerate.loss", loss, ref_loss)
      _gate(f"lambda_weight.{kind_name}.degenerate.dscores", grad, ref_grad)


# ---- 5. list weights and reductions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_list_weights_and_reductions(kind_name):
  B, L = 67, 33
  y, s = _inputs(B, L)
  cfg = lam.configs(L)["mu0.25"]
  ref_loss, ref_grad = _reference(kind_name, "mu0.25", B, L)
  w = (np.random.RandomState(3).rand(B) + 0.5).astype(np.float32)
  for reduction, factor in (("none", 1.0), ("sum", 1.0), ("sum_over_batch_size", 1.0 / B)):
    for weight in (w, w[:, None]):
      loss, grad = _run(kind_name, cfg, y, s, weight=weight, reduction=reduction)
      wl = lw.Entry(ref_loss.value * w, ref_loss.n, ref_loss.yard * w, ref_loss.u + 1.0)
      if reduction == "none":
        _gate(f"lambda_weight.{kind_name}.weighted.loss", loss, wl)
      else:       # one more sum over the B lists: B - 1 more additions, one more product
        tot = lw.Entry(wl.value.sum() * factor, ref_loss.n.max() + B, wl.yard.sum() * factor, float(ref_loss.u.max()) + 2.0)
        assert loss.shape == ()
        _gate(f"lambda_weight.{kind_name}.{reduction}.loss", loss, tot)
      sc = (w * factor)[:, None]
      _gate(f"lambda_weight.{kind_name}.weighted.dscores", grad,
            lw.Entry(ref_grad.value * sc, ref_grad.n, ref_grad.yard * sc, ref_grad.u + 2.0))


# ---- 6. reproducibility; None is the old route -------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(67, 5), (67, 64), (67, 130), (3, 1024)])
def test_two_calls_give_identical_bits(B, L):
  y, s = _inputs(B, L)
  for kind_name in KIND_NAMES:
    for cfg in (lam.Config(None, True, 0.0), lam.Config(3, True, 0.25)):
      a, b = _run(kind_name, cfg, y, s), _run(kind_name, cfg, y, s)
      np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
      np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("B,L", [(67, 5), (3, 64), (3, 257)])
def test_lambda_weight_none_is_the_loss_without_the_argument(B, L):
  y, s = _inputs(B, L)
  for kind_name in KIND_NAMES:
    out = []
    for loss_fn in (_loss_class(kind_name)(reduction="none"), _loss_class(kind_name)(reduction="none", lambda_weight=None)):
      yt, st = _cuda(y), _cuda(s).requires_grad_(True)
      v = loss_fn(yt, st)
      v.sum().backward()
      out.append((_bits(v), _bits(st.grad)))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    weighted, _ = _run(kind_name, lam.Config(None, True, 0.0), y, s)
    assert not np.array_equal(weighted.view(np.uint32), out[0][0])


# ---- 7. no L^2 memory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", KIND_NAMES)
def test_weighted_losses_allocate_no_pair_matrix(kind_name):
  """B = 64, L = 1024: a [B, L, L] float32 temporary would be 256 MiB; forward + backward may add 8 B L 4 bytes + 1 MiB
  (the measurement of tests/test_listwise_gpu.py)."""
  from recommenders_amd import losses
  B, L = 64, 1024
  yt = _cuda(lw.make_labels(B, L, 5))
  st = _cuda(lw.make_scores(B, L, 5)).requires_grad_(True)
  loss_fn = _loss_class(kind_name)(lambda_weight=losses.NDCGLambdaWeight(topn=10, smooth_fraction=0.25))
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


# ---- 8. captured step --------------------------------------------------------------------------------------------------
def test_captured_step_replays_the_eager_trajectory_bit_for_bit():
  import recommenders_amd as tfrs
  B, L = 48, 9

  class Ranker(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.items = tfrs.layers.embedding.Embedding(500, 16)
      self.score = tfrs.layers.blocks.Dense(1)
      loss = tfrs.losses.PairwiseLogisticLoss(lambda_weight=tfrs.losses.NDCGLambdaWeight(topn=5))
      self.task = tfrs.tasks.Ranking(loss=loss)

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
  step = graphed.make_graphed_train_step(batches[0])
  for a, b in zip(eager.parameters(), graphed.parameters()):      # warm-up rolled back
    np.testing.assert_array_equal(_bits(a), _bits(b))
  start = [p.detach().clone() for p in eager.parameters()]
  for batch in batches:
    le, lg = eager.train_step(batch), step(batch)
    assert float(le["loss"]) == float(lg["loss"]) and float(le["loss"]) > 0.0
  for a, b, s0 in zip(eager.parameters(), graphed.parameters(), start):
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not torch.equal(a, s0)


# ---- 9. C entries on the device ----------------------------------------------------------------------------------------
def test_c_entries_skip_empty_batches_and_the_classes_handle_them():
  from recommenders_amd import _lib, losses
  lib = _lib.load()
  buf = torch.zeros(64, device="cuda")
  p, stream = _lib.ptr(buf), _lib.current_stream()
  assert lib.tfrs_listwise_lambda_fwd(1, None, None, 0, 5, 3, 1, 0.25, None, stream) == _lib.TFRS_OK
  assert lib.tfrs_listwise_lambda_bwd(2, None, None, 0, 5, 0, 0, 0.0, None, None, stream) == _lib.TFRS_OK
  assert lib.tfrs_listwise_lambda_fwd(0, p, p, 2, 5, 0, 1, 0.0, p, stream) == _lib.TFRS_EINVAL
  assert lib.tfrs_listwise_lambda_bwd(1, p, p, 2, 5, 0, 1, float("nan"), p, p, stream) == _lib.TFRS_EINVAL
  torch.cuda.synchronize()
  assert not buf.any()
  empty_y, empty_s = torch.zeros(0, 5, device="cuda"), torch.zeros(0, 5, device="cuda", requires_grad=True)
  w = losses.NDCGLambdaWeight(topn=3, smooth_fraction=0.5)
  assert losses.PairwiseHingeLoss(reduction="none", lambda_weight=w)(empty_y, empty_s).shape == (0,)
  out = losses.PairwiseLogisticLoss(lambda_weight=w)(empty_y, empty_s)
  out.backward()
  assert float(out.detach()) == 0.0 and empty_s.grad.shape == (0, 5)
