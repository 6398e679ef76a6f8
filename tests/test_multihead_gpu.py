"""Multi-head (max-sim) queries on the GPU: the fused in-batch softmax kernels (tfrs_inbatch_softmax_mh_ce_fwd/_bwd)
against the float64 restatement at the layout edges of the head groups, the routing of ``tasks.Retrieval`` and the
multi-head exact top-K of ``BruteForce`` (tfrs_topk_merge_heads) against the oracle's scores, compared with ``==``.

Inputs of the big case lists lie on the grid {-2 .. 2} / 4: every dot product is then exact in float32 in any
summation order, so the winning head of every pair -- and every tie between heads -- is decided exactly, on the
device as in float64.  Random normal inputs are used only behind a host-side guard on the gap between a pair's two
best heads (tests/multihead_restatement.py head_gap_guard).

Tolerance of the gradients: the gate the 2-D f32-MFMA path is held to (test_ops_gpu.py GATE_SOFTMAX_GRAD["f32"]
capped by 4 x the frozen observation of tests/golden/float_gates.json, as tests/conftest.py float_gate does for
"softmax_f32.dq" / ".dc"), in units of the restatement's yardsticks: 2.7e-6 for dq, 3.5e-6 for dc.  Observed on MI355X over
every case of this file: dq 1.4e-6, dc 5.7e-7, loss 5.8e-7 relative (limit 1e-5), so no wider gate was needed."""

import numpy as np
import pytest

from oracle import topk as o_topk
from tests import multihead_restatement as mh
from tests.conftest import float_gate, load_golden
from tests.softmax_handbuilt import entry_point_outputs as _entry_point_outputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_FROZEN = load_golden("float_gates.json")["gates"]
GATE = {"dq": min(3.5e-6, 4.0 * _FROZEN["softmax_f32.dq"]), "dc": min(3.5e-6, 4.0 * _FROZEN["softmax_f32.dc"])}
LOSS_RTOL = 1e-5                       # the 2-D tests' loss tolerance (test_inbatch_softmax_options_vs_oracle)


def _t(a, **kw):
  return torch.as_tensor(np.asarray(a), **kw).cuda()


def _np(x):
  return x.detach().cpu().numpy()


def _padded(heads):
  hp = 1
  while hp < heads:
    hp *= 2
  return hp


def _grid(rng, shape):
  return (rng.integers(-2, 3, size=shape) / 4.0).astype(np.float32)


def _option_variants(rng, nq, nc):
  w = rng.uniform(0.1, 2.0, size=nq).astype(np.float32)
  p = rng.uniform(0.0, 1.0, size=nc).astype(np.float32)
  p[::7] = 0.0                                          # the 1e-6 clip
  ids = rng.integers(0, max(nc // 3, 2), size=nc)       # duplicates: accidental hits
  mask = rng.uniform(size=(nq, nc)) > 0.2
  mask[np.arange(nq), np.arange(nq)] = True
  return {"plain": dict(), "weights": dict(sample_weight=w), "temperature": dict(temperature=0.7),
          "correction": dict(candidate_sampling_probability=p), "accidental_hits": dict(candidate_ids=ids),
          "mask": dict(score_mask=mask),
          "all": dict(sample_weight=w, temperature=1.3, candidate_sampling_probability=p, candidate_ids=ids,
                      score_mask=mask)}


def _run_functional(q3, c, kw, upstream=2.0):
  """(loss, dq, dc) of the fused functional, with an upstream gradient other than 1 divided out again."""
  from recommenders_amd.tasks.retrieval import multi_head_in_batch_softmax_loss
  tq, tc = _t(q3).requires_grad_(True), _t(c).requires_grad_(True)
  loss = multi_head_in_batch_softmax_loss(tq, tc, **{k: _t(v) if isinstance(v, np.ndarray) else v
                                                     for k, v in kw.items()})
  (loss * upstream).backward()
  return float(loss), _np(tq.grad) / upstream, _np(tc.grad) / upstream


def _check_against_restatement(q3, c, kw, tag):
  ref = mh.loss(q3, c, **kw)
  dq_ref, dc_ref, dq_y, dc_y = mh.loss_grads(q3, c, return_yardsticks=True, **kw)
  loss, dq, dc = _run_functional(q3, c, kw)
  err = abs(loss - ref) / max(abs(ref), 1e-30)
  eq = float_gate("softmax_mh.dq", dq, dq_ref, dq_y, GATE["dq"])
  ec = float_gate("softmax_mh.dc", dc, dc_ref, dc_y, GATE["dc"])
  print(f"{tag}: loss rel err {err:.3e}, dq {eq:.3e}, dc {ec:.3e} (yardstick units)")
  assert err <= LOSS_RTOL, (tag, loss, ref)
  return dq, dc


def _heads_all_win_and_tie(q3, c):
  dots = mh.head_dots(q3, c)
  wins = np.bincount(dots.argmax(axis=1).ravel(), minlength=q3.shape[1])
  if q3.shape[1] == 1:
    return True, False
  top2 = np.sort(dots, axis=1)[:, -2:, :]
  return bool(np.all(wins > 0)), bool(np.any(top2[:, 0] == top2[:, 1]))


def _grid_inputs(nq, heads, nc, d, need_conditions):
  """Grid inputs; for ``need_conditions`` the first seed at which every head wins a pair and some pair is tied."""
  for seed in range(4000):
    rng = np.random.default_rng([seed, nq, heads, nc, d])
    q3, c = _grid(rng, (nq, heads, d)), _grid(rng, (nc, d))
    if not need_conditions:
      return rng, q3, c
    all_win, tie = _heads_all_win_and_tie(q3, c)
    if all_win and (tie or heads == 1):
      return rng, q3, c
  raise AssertionError(f"no seed gives every head a win and a tie at {(nq, heads, nc, d)}")


HEADS = (1, 2, 3, 4, 5, 8, 16, 32)
DIMS = (1, 16, 20, 64, 100, 128)


def _grid_cases():
  """(heads, nq, nc, d) paired, not crossed: nq at the wave's query boundary (32 / Hp queries per wave), nc at the
  tile / split boundary of the candidate side (at these sizes every 32-row tile is a split of its own, so 33 and 65
  are one row past a split boundary), d over every padded width and a non-multiple of 4."""
  cases = []
  for i, heads in enumerate(HEADS):
    qw = 32 // _padded(heads)
    seen = set()
    for jn, (nq, nc) in enumerate(((qw - 1, 64), (qw, 65), (qw + 1, None), (1, 33), (2 * qw + 1, 0))):
      if nq < 1 or nq in seen:
        continue
      seen.add(nq)
      nc = nq + 1 if nc is None else max(nc, nq)
      d = DIMS[(i + jn) % len(DIMS)]
      if d == 1 and 2 < heads <= 8:       # five grid values cannot keep more than two heads distinct at d = 1
        d = 20
      cases.append((heads, nq, nc, d))
  cases.append((2, 17, 40, 1))
  cases.append((1, 33, 33, 1))
  return cases


@pytest.mark.parametrize("index,case", list(enumerate(_grid_cases())), ids=lambda v: str(v).replace(" ", ""))
def test_exact_grid_cases_against_the_restatement(index, case):
  heads, nq, nc, d = case
  rng, q3, c = _grid_inputs(nq, heads, nc, d, need_conditions=heads <= 8)
  variants = _option_variants(rng, nq, nc)
  names = list(variants)
  name = "plain" if index % 2 == 0 else names[1 + (index // 2) % (len(names) - 1)]     # every other case is PLAIN
  _check_against_restatement(q3, c, variants[name], f"grid{case}/{name}")


def test_dc_split_boundary_of_the_streamed_query_side():
  """The dc kernel streams the flat (query, head) slots: with 683 candidate blocks the planner asks for 3 splits of
  the 5 query tiles (H = 32: one query per tile) -- 2 + 2 + 1, the last split one query past a split boundary."""
  heads, nq, nc, d = 32, 5, 683 * 32, 16
  rng, q3, c = _grid_inputs(nq, heads, nc, d, need_conditions=False)
  _check_against_restatement(q3, c, dict(temperature=2.0), "dc_split")


@pytest.mark.parametrize("heads,nq,nc,d", [(3, 9, 41, 20), (8, 5, 70, 64)])
def test_each_logit_option_alone_and_all_together(heads, nq, nc, d):
  rng, q3, c = _grid_inputs(nq, heads, nc, d, need_conditions=True)
  for name, kw in _option_variants(rng, nq, nc).items():
    _check_against_restatement(q3, c, kw, f"options({heads},{nq},{nc},{d})/{name}")


@pytest.mark.parametrize("nq,heads,nc,d", [(48, 3, 60, 16), (70, 2, 130, 20)])
def test_random_normal_inputs_behind_the_gap_guard(nq, heads, nc, d):
  for seed in range(100):
    rng = np.random.default_rng([seed, nq, heads])
    q3 = rng.normal(size=(nq, heads, d)).astype(np.float32)
    c = rng.normal(size=(nc, d)).astype(np.float32)
    gap, bound = mh.head_gap_guard(q3, c)
    if gap >= bound:
      break
  print(f"seed {seed}: smallest head gap {gap:.3e}, bound {bound:.3e}")
  assert gap >= bound
  variants = _option_variants(rng, nq, nc)
  for name in ("plain", "all"):
    _check_against_restatement(q3, c, variants[name], f"normal({nq},{heads},{nc},{d})/{name}")


@pytest.mark.parametrize("heads,d,used_blocks", [(4, 16, (0, 1, 2)), (5, 20, (0, 2, 4))])
def test_a_head_that_never_wins_gets_exactly_zero(heads, d, used_blocks):
  """Planted winners: head h lives on coordinates [4h, 4h + 4), every candidate on one block, all entries positive:
  the head of a candidate's block wins the pair strictly, the heads of unused blocks never win."""
  rng = np.random.default_rng(heads)
  nq, nc = 11, 37
  q3 = np.zeros((nq, heads, d), np.float32)
  for h in range(heads):
    q3[:, h, 4 * h:4 * h + 4] = rng.integers(1, 3, size=(nq, 4)) / 4.0
  c = np.zeros((nc, d), np.float32)
  block = np.asarray(used_blocks)[rng.integers(0, len(used_blocks), size=nc)]
  for j in range(nc):
    c[j, 4 * block[j]:4 * block[j] + 4] = rng.integers(1, 3, size=4) / 4.0
  _, hstar = mh.winners(q3, c)
  assert np.array_equal(hstar, np.broadcast_to(block, (nq, nc)))
  dq, _ = _check_against_restatement(q3, c, dict(temperature=0.5), "planted")
  for h in range(heads):
    if h in used_blocks:
      assert np.abs(dq[:, h]).sum() > 0
    else:
      assert np.all(dq[:, h] == 0.0), h


def test_ties_go_to_the_lowest_head():
  """Duplicated heads (the later copy gets exactly nothing) and all-zero queries (every head ties at 0: head 0)."""
  rng = np.random.default_rng(21)
  nq, heads, nc, d = 19, 3, 45, 20
  q3, c = _grid(rng, (nq, heads, d)), _grid(rng, (nc, d))
  q3[:, 1] = q3[:, 0]
  q3[5] = 0.0
  q3[18] = 0.0
  dq, _ = _check_against_restatement(q3, c, dict(), "ties")
  assert np.all(dq[:, 1] == 0.0)
  assert np.all(dq[[5, 18], 1:] == 0.0) and np.abs(dq[[5, 18], 0]).sum() > 0
  # random normal heads: a bit-identical copy still ties exactly (the same arithmetic in another lane)
  q3 = rng.normal(size=(nq, 2, d)).astype(np.float32)
  q3[:, 1] = q3[:, 0]
  _, dq, _ = _run_functional(q3, rng.normal(size=(nc, d)).astype(np.float32), dict())
  assert np.all(dq[:, 1] == 0.0) and np.abs(dq[:, 0]).sum() > 0


# ------------------------------------------------------------------------------------------ one head = the 2-D kernels
ROUTE_SHAPES = ((5, 5, 8),          # one partial tile
                (33, 70, 20),       # a second row block with one valid row, a ragged last tile, a padded dim
                (64, 97, 128))      # DP = 128, two full row blocks


def _routes_at(shape):
  """{variant: (multi-head outputs, 2-D outputs)} for random normal inputs of ``shape``, plain and with every option."""
  nq, nc, d = shape
  rng = np.random.default_rng([nq, nc, d])
  q = rng.normal(size=(nq, d)).astype(np.float32)
  c = rng.normal(size=(nc, d)).astype(np.float32)
  variants = _option_variants(rng, nq, nc)
  return {name: (_entry_point_outputs(q, c, variants[name], True), _entry_point_outputs(q, c, variants[name], False))
          for name in ("plain", "all")}


def _assert_routes_identical(shape):
  for variant, (mh_out, flat_out) in _routes_at(shape).items():
    for what, a, b in zip(("loss", "lse", "dq", "dc"), mh_out, flat_out):
      assert np.all(np.isfinite(a)), (shape, variant, what)
      np.testing.assert_array_equal(a, b, err_msg=f"{shape}/{variant}/{what}")


@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_one_head_through_the_multi_head_entry_points_is_the_2d_f32_route_bit_for_bit(shape, monkeypatch):
  """``[B, 1, D]`` queries through tfrs_inbatch_softmax_mh_ce_fwd/_bwd against ``[B, D]`` queries through
  tfrs_inbatch_softmax_ce_fwd/_bwd on the f32 kernels: the two instantiations (MH = true at one head, MH = false) of
  the one kernel source do the same arithmetic in the same order, so loss, lse, dq and dc are equal bit for bit."""
  monkeypatch.setenv("TFRS_SOFTMAX_MODE", "f32")
  _assert_routes_identical(shape)


def test_one_head_equals_the_2d_f32_route_with_more_splits_asked_for():
  """The same at (33, 70, 20) under TFRS_SOFTMAX_WAVES=4096 (the split planner reads the option on every call)."""
  from recommenders_amd import _lib
  try:
    _lib.set_option("TFRS_SOFTMAX_WAVES", "4096")
    _lib.set_option("TFRS_SOFTMAX_MODE", "f32")
    _assert_routes_identical((33, 70, 20))
  finally:
    _lib.set_option("TFRS_SOFTMAX_WAVES", None)
    _lib.set_option("TFRS_SOFTMAX_MODE", None)


# ------------------------------------------------------------------------------------------ Retrieval routing
class _Counter:
  def __init__(self, fn):
    self.fn, self.calls = fn, 0

  def __call__(self, *args):
    self.calls += 1
    return self.fn(*args)


def _refuse(*args, **kwargs):
  raise AssertionError("the explicit score matrix was built")


def test_retrieval_sends_multi_head_queries_to_the_fused_kernels(monkeypatch):
  import recommenders_amd as tfrs
  from recommenders_amd import _lib
  from recommenders_amd.tasks import retrieval as rt
  lib = _lib.load()
  fwd = _Counter(lib.tfrs_inbatch_softmax_mh_ce_fwd)
  bwd = _Counter(lib.tfrs_inbatch_softmax_mh_ce_bwd)
  monkeypatch.setattr(lib, "tfrs_inbatch_softmax_mh_ce_fwd", fwd)
  monkeypatch.setattr(lib, "tfrs_inbatch_softmax_mh_ce_bwd", bwd)
  rng = np.random.default_rng(31)
  nq, heads, nc, d = 40, 3, 52, 16
  q3, c = _grid(rng, (nq, heads, d)), _grid(rng, (nc, d))
  v = _option_variants(rng, nq, nc)["all"]
  task = tfrs.tasks.Retrieval(temperature=v["temperature"], remove_accidental_hits=True)
  call_kw = dict(sample_weight=_t(v["sample_weight"]), candidate_ids=_t(v["candidate_ids"]),
                 candidate_sampling_probability=_t(v["candidate_sampling_probability"]),
                 score_mask=_t(v["score_mask"]), compute_metrics=False)
  with monkeypatch.context() as m:
    m.setattr(rt, "_DenseFn", type("NoDense", (), {"apply": staticmethod(_refuse)}))
    m.setattr(lib, "tfrs_compute_scores", _refuse)
    tq, tc = _t(q3).requires_grad_(True), _t(c).requires_grad_(True)
    loss = task(tq, tc, **call_kw)
    loss.backward()
  assert (fwd.calls, bwd.calls) == (1, 1)
  fl, fdq, fdc = _run_functional(q3, c, v, upstream=1.0)
  assert float(loss) == fl
  np.testing.assert_array_equal(_np(tq.grad), fdq)
  np.testing.assert_array_equal(_np(tc.grad), fdc)
  # factorized metrics stay skipped for 3-D queries (reference :216): compute_metrics=True changes nothing
  task_m = tfrs.tasks.Retrieval(metrics=tfrs.metrics.FactorizedTopK(candidates=[c], ks=[1]))
  fused_calls = fwd.calls
  task_m(_t(q3), _t(c))
  assert fwd.calls == fused_calls + 1
  fused_calls = fwd.calls
  # a user loss, hard negatives, batch metrics, more than 32 heads: the explicit route, as before
  from recommenders_amd.tasks.retrieval import TopKCategoricalAccuracy
  user_loss = lambda y_true, y_pred, sample_weight=None: rt.logits_softmax_ce_sum(y_pred, y_true, sample_weight)
  wide_heads = _grid(rng, (nq, 33, d))
  for explicit, queries in ((tfrs.tasks.Retrieval(loss=user_loss), q3),
                            (tfrs.tasks.Retrieval(num_hard_negatives=5), q3),
                            (tfrs.tasks.Retrieval(batch_metrics=[TopKCategoricalAccuracy(k=3)]), q3),
                            (tfrs.tasks.Retrieval(), wide_heads)):
    dense = _Counter(rt._DenseFn.apply)
    with monkeypatch.context() as m:
      m.setattr(rt, "_DenseFn", type("CountDense", (), {"apply": staticmethod(dense)}))
      got = explicit(_t(queries), _t(c), compute_metrics=False)
    assert dense.calls == 1 and fwd.calls == fused_calls
    if explicit._num_hard_negatives is None:
      assert float(got) == pytest.approx(mh.loss(queries, c), rel=LOSS_RTOL)


def test_captured_train_step_replays_the_multi_head_route():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(3)
  heads, d = 3, 32

  class MultiInterest(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.user_model = tfrs.layers.embedding.Embedding(943, heads * d)
      self.item_model = tfrs.layers.embedding.Embedding(1682, d)
      self.task = tfrs.tasks.Retrieval(temperature=0.5)

    def compute_loss(self, features, training=False):
      users = self.user_model(features["user_id"]).reshape(-1, heads, d)
      return self.task(users, self.item_model(features["movie_id"]), compute_metrics=False)

  def make():
    torch.manual_seed(5)
    m = MultiInterest()
    m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.5))
    return m

  batches = [{"user_id": _t(rng.integers(0, 943, size=300)),
              "movie_id": _t(rng.integers(0, 1682, size=300))} for _ in range(3)]
  eager, graphed = make(), make()
  step = graphed.make_graphed_train_step(batches[0])
  for batch in batches + batches:
    le = eager.train_step(batch)
    lg = step(batch)
    assert float(le["loss"]) == float(lg["loss"])
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a), _np(b))


# ------------------------------------------------------------------------------------------ BruteForce
N_ROWS = 2000
_CORPUS = {}


def _corpus(d):
  if d not in _CORPUS:
    _CORPUS[d] = np.random.default_rng(d).normal(size=(N_ROWS, d)).astype(np.float32)     # shared, never written
  return _CORPUS[d]


def _related_heads(rng, nq, heads, d, spread=0.5):
  """Heads of a query around a common direction: their top-k lists overlap without being equal."""
  base = rng.normal(size=(nq, 1, d))
  return (base + spread * rng.normal(size=(nq, heads, d))).astype(np.float32)


def _brute_force(c, k=10):
  import recommenders_amd as tfrs
  return tfrs.layers.factorized_top_k.BruteForce(k=k).index(_t(c))


@pytest.mark.parametrize("heads,k,d", [(1, 10, 20), (2, 1, 64), (3, 256, 128), (8, 10, 64), (32, 256, 20),
                                       (8, 1024, 128), (32, 1, 128), (3, 10, 64), (8, 10, 20), (2, 256, 64)])
def test_multi_head_top_k_equals_the_restatement(heads, k, d):
  nq = 21
  c = _corpus(d)
  q3 = _related_heads(np.random.default_rng([heads, k, d]), nq, heads, d)
  want_s, want_r = mh.topk(q3, c, k)
  # what the inputs exercise, checked on the host
  hs = mh.head_scores(q3, c)                                             # [B, H, N]
  winner = hs.argmax(axis=1)                                             # [B, N]
  top_winner = np.take_along_axis(winner, want_r, axis=1)                # head behind every returned row
  if heads <= k * nq:
    assert set(np.unique(top_winner)) == set(range(heads)), "every head contributes"
  if k >= 10 and heads >= 3:
    assert all(len(set(row)) >= 2 for row in top_winner), "every query's top-k mixes heads"
  if heads >= 2 and k >= 10:
    lists = np.argsort(-hs, axis=2, kind="stable")[:, :, :k]
    repeats = [heads * k - len(np.unique(lists[b])) for b in range(nq)]
    print(f"rows shared between the per-head lists, per query: {min(repeats)} .. {max(repeats)}")
    assert min(repeats) >= 1, "the duplicate collapse is exercised for every query"
  scores, ids = _brute_force(c)(_t(q3), k=k)
  np.testing.assert_array_equal(_np(ids), want_r)
  np.testing.assert_array_equal(_np(scores), want_s)


def test_multi_head_top_k_edge_inputs():
  d, k = 64, 10
  rng = np.random.default_rng(77)
  c = _corpus(d).copy()
  c[100:200] = c[:100]                                                   # exact duplicate rows: lower row first
  layer = _brute_force(c, k=k)
  q = rng.normal(size=(9, d)).astype(np.float32)
  q[:3] = c[[5, 50, 99]] * 3                                             # their best rows are duplicated ones
  # identical heads: every row of every list repeated H times
  q3 = np.repeat(q[:, None, :], 4, axis=1)
  want_s, want_r = o_topk.top_k(o_topk.scores(q, c), k)
  scores, ids = layer(_t(q3))
  np.testing.assert_array_equal(_np(ids), want_r)
  np.testing.assert_array_equal(_np(scores), want_s)
  assert any(r0 + 100 == r1 for r0, r1 in zip(want_r[0][:-1], want_r[0][1:]))    # a duplicate pair, in row order
  # related heads on the duplicated corpus, with exclusions
  q3 = _related_heads(rng, 9, 3, d)
  want_s, want_r = mh.topk(q3, c, k)
  scores, ids = layer(_t(q3))
  np.testing.assert_array_equal(_np(ids), want_r)
  np.testing.assert_array_equal(_np(scores), want_s)
  excl = np.concatenate([want_r[:, [0, 3]], np.full((9, 1), 1999)], axis=1)      # two of the top rows and a far one
  wide_s, wide_r = mh.topk(q3, c, k + 3)
  want_s, want_r = o_topk.exclude(wide_s, wide_r, excl, k)
  scores, ids = layer.query_with_exclusions(_t(q3), _t(excl), k=k)
  np.testing.assert_array_equal(_np(ids), want_r)
  np.testing.assert_array_equal(_np(scores), want_s)
  # graphed call: replay == eager, also on new queries
  graphed = layer.make_graphed_call(_t(q3), k=k)
  for queries in (q3, _related_heads(rng, 9, 3, d)):
    es, ei = layer(_t(queries))
    gs, gi = graphed(_t(queries))
    np.testing.assert_array_equal(_np(gi), _np(ei))
    np.testing.assert_array_equal(_np(gs), _np(es))
  # outside the envelope: the limit is named
  with pytest.raises(ValueError, match="8192"):
    layer(_t(_related_heads(rng, 2, 25, d)), k=328)                      # H * k = 8200
  with pytest.raises(ValueError, match="32 heads"):
    layer(_t(_related_heads(rng, 2, 33, d)), k=5)
  with pytest.raises(ValueError, match="1024"):
    layer(_t(q3), k=1025)
  with pytest.raises(ValueError, match="dimension"):
    layer(_t(_related_heads(rng, 2, 3, d + 1)), k=5)
