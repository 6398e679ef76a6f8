"""The list metrics on the MI355X (``listwise_metrics_kernel`` of csrc/listwise.hip through ``tfrs_listwise_metrics``,
metrics/listwise.py and tasks/ranking.py) against the restatement of tests/listwise_metrics_restatement.py: the
integer-valued metrics bit for bit (one correctly rounded division of two exact integers, as
tests/test_listwise_metrics_host.py argues), MAP / DCG / ARP under the bounds derived there (``float_gate`` with limit
eps, the bound as yardstick and a floor of one smallest normal float).

Shapes: ``lw.SHAPES`` -- B in {1, 3, 67} x L in {1, 2, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 256, 257, 1024} (B = 3
only at 1024): both sides of every switch of the work mapping, one and several workgroups, the top of the envelope."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import listwise_metrics_restatement as lm
from tests import listwise_restatement as lw
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

GATE_FLOOR = lw.FLOOR / lw.EPS
TOPNS = (None, 1, 10, 2000)
NAMES = {v: k for k, v in lm.KINDS.items()}


def _cuda(a):
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(a):
  if isinstance(a, torch.Tensor):
    a = a.detach().cpu().contiguous().numpy()
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _call(y, s, descriptors):
  """(values, weights), each [len(descriptors), B] float32, straight from the C entry; descriptors = (kind, topn)."""
  from recommenders_amd import _lib
  yt, st = _cuda(y), _cuda(s)
  n = len(descriptors)
  out = torch.full((2, n, y.shape[0]), -7.0, device="cuda")
  kinds = (ctypes.c_int * n)(*[k for k, _ in descriptors])
  topns = (ctypes.c_int * n)(*[0 if t is None else t for _, t in descriptors])
  _lib.check(_lib.load().tfrs_listwise_metrics(_lib.ptr(yt), _lib.ptr(st), y.shape[0], y.shape[1], n, kinds, topns,
                                               _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.current_stream()))
  out = out.cpu().numpy()
  return out[0], out[1]


def _classes():
  from recommenders_amd import metrics
  return {lm.NDCG: metrics.NDCGMetric, lm.DCG: metrics.DCGMetric, lm.MRR: metrics.MRRMetric, lm.HITS: metrics.HitsMetric,
          lm.PRECISION: metrics.PrecisionMetric, lm.RECALL: metrics.RecallMetric,
          lm.MAP: metrics.MeanAveragePrecisionMetric, lm.ARP: metrics.ARPMetric, lm.OPA: metrics.OPAMetric}


def _make(kind, topn):
  return _classes()[kind]() if kind in lm.UNCUT_KINDS else _classes()[kind](topn=topn)


def _check(y, s, descriptors, what):
  """Every descriptor of one call against the restatement: integer kinds bit for bit in value and weight, rounded
  kinds under their bounds; every weight bit for bit where all valid labels are integers (ARP's sum of labels is then
  exact in any order, as the restatement argues), else where the restatement's weight bound is 0; a list that does
  not count stores +0."""
  values, weights = _call(y, s, descriptors)
  integer_labels = bool(np.all(y[y >= 0] == np.round(y[y >= 0])))
  for m, (kind, topn) in enumerate(descriptors):
    ref = lm.BatchMetric(kind, y, s, topn)
    tag = f"{what} {NAMES[kind]} topn={topn}"
    if kind in lm.INTEGER_KINDS:
      np.testing.assert_array_equal(_bits(values[m]), _bits(ref.f32), err_msg=tag)
      np.testing.assert_array_equal(_bits(weights[m]), _bits(ref.weight), err_msg=tag)
    else:
      err = float_gate(f"listwise_metrics.{NAMES[kind]}.lists", values[m], ref.value, ref.value_bound / lw.EPS, lw.EPS,
                       floor=GATE_FLOOR)
      print(f"{tag}: error {err / lw.EPS:.3g} of the bound")
      assert not integer_labels or (ref.weight_bound == 0.0).all(), tag
      if integer_labels or (ref.weight_bound == 0.0).all():
        np.testing.assert_array_equal(_bits(weights[m]), _bits(ref.weight), err_msg=tag)
      else:
        float_gate(f"listwise_metrics.{NAMES[kind]}.weights", weights[m], ref.weight, ref.weight_bound / lw.EPS, lw.EPS,
                   floor=GATE_FLOOR)
    assert not _bits(values[m])[ref.weight == 0.0].any(), tag          # +0 where the list does not count
  return values, weights


@functools.lru_cache(maxsize=None)
def _inputs(B, L, labels="graded"):
  seed = 500 * L + B
  make = {"graded": lw.make_labels, "sparse": lm.make_sparse_binary_labels, "half": lm.make_half_labels}[labels]
  y, s = make(B, L, seed), lw.make_grid_scores(B, L, seed, step=0.5, lim=3.0)
  if L >= 2:                           # planted tie at the head of every list
    s[:, 1] = s[:, 0]
  return y, s


# ---- 1. integer-valued metrics, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
def test_integer_valued_metrics_are_bit_equal(B, L):
  """MRR, hits, precision, recall at every topn and OPA, on grid scores (ties by construction), graded and sparse
  binary labels: np.float32(num) / np.float32(den) bit for bit, weights included."""
  desc = [(k, t) for k in (lm.MRR, lm.HITS, lm.PRECISION, lm.RECALL) for t in TOPNS]      # 16 descriptors
  for labels in ("graded", "sparse"):
    y, s = _inputs(B, L, labels)
    _check(y, s, desc, f"B={B} L={L} {labels}")
    _check(y, s, [(lm.OPA, None)], f"B={B} L={L} {labels}")


# ---- 2. rounded metrics under the restatement's bound --------------------------------------------------------------------
@pytest.mark.parametrize("B,L", lw.SHAPES)
def test_rounded_metrics_stay_under_the_bound(B, L):
  """MAP and DCG at every topn and ARP: graded labels on grid scores, labels with 0.5 on continuous scores."""
  desc = [(k, t) for k in (lm.MAP, lm.DCG) for t in TOPNS] + [(lm.ARP, None)]
  y, s = _inputs(B, L, "graded")
  _check(y, s, desc, f"B={B} L={L} graded")
  y = _inputs(B, L, "half")[0]
  _check(y, lw.make_scores(B, L, 500 * L + B), desc, f"B={B} L={L} half")


# ---- 3. planted edges ----------------------------------------------------------------------------------------------------
def _ranked(L, labels_by_rank, seed):
  """One list whose sorted rank r sits at position perm[r] (a random permutation; scores distinct multiples of 1/4)
  and carries labels_by_rank.get(r, 0)."""
  perm = np.random.RandomState(seed).permutation(L)
  y, s = np.zeros(L, dtype=np.float32), np.zeros(L, dtype=np.float32)
  for r in range(L):
    s[perm[r]] = 0.25 * (L - r)
    y[perm[r]] = labels_by_rank.get(r, 0.0)
  return y, s


CUT_DESC = lambda topn: [(k, topn) for k in (lm.MRR, lm.HITS, lm.PRECISION, lm.RECALL, lm.MAP, lm.DCG, lm.NDCG)]


@pytest.mark.parametrize("L,topn", [(9, 3), (64, 10), (130, 64), (1024, 256), (1024, 768)])
def test_planted_cut_and_tie_edges(L, topn):
  """The only relevant item at sorted rank topn - 1 (inside the cut) and at rank topn (outside); two tied scores
  straddling the cut with the relevant item at the later position (outside) and at the earlier one (inside).  At
  L = 1024 the ranks 255 / 256 and 767 / 768 change owner thread and item slot."""
  rows = [_ranked(L, {topn - 1: 1.0}, 1), _ranked(L, {topn: 1.0}, 2)]
  for later in (True, False):
    y, s = _ranked(L, {}, 3)
    order = lw.score_order(y, s)
    a, b = sorted((order[topn - 1], order[topn]))          # positions of the two ranks around the cut
    s[a] = s[b] = s[order[topn - 1]]                       # tied: position a takes rank topn - 1, b rank topn
    y[b if later else a] = 1.0
    rows.append((y, s))
  y, s = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
  values, weights = _check(y, s, CUT_DESC(topn), f"L={L}")
  inside = np.array([1.0, 0.0, 0.0, 1.0], dtype=np.float32)
  np.testing.assert_array_equal(values[1], inside)                                             # hits
  np.testing.assert_array_equal(values[0], inside / np.float32(topn))                          # MRR = MAP = 1 / topn
  np.testing.assert_array_equal(values[4], inside / np.float32(topn))
  np.testing.assert_array_equal(values[2], inside / np.float32(topn))                          # precision = 1 / topn
  np.testing.assert_array_equal(values[3], inside)                                             # recall
  np.testing.assert_array_equal(weights[:5], np.ones((5, 4), dtype=np.float32))


@pytest.mark.parametrize("L", [5, 64, 257, 1024])
def test_planted_degenerate_lists(L):
  B = 8
  y, s = lw.make_labels(B, L, 61 + L), lw.make_grid_scores(B, L, 61 + L)
  y[0, 0] = 2.0
  y[1] = np.where(y[1] >= 0, 1.0 + (np.arange(L) % 3), -1.0)      # all items relevant
  y[1, 0] = 1.0
  y[2] = np.where(y[2] >= 0, 0.0, -1.0)                           # none relevant, no gain
  y[2, 0] = 0.0
  y[3] = -1.0                                                     # all padding
  y[4] = -1.0
  y[4, L // 2] = 3.0                                              # one valid item
  y[5] = np.where(y[5] >= 0, 0.0, -1.0)                           # 0.5: R = 0, but gain, relevance mass and pairs
  y[5, 0], y[5, L - 1] = 0.5, 0.0
  if L >= 4:
    y[6, L - L // 4:] = -1.0                                      # n < topn (topn = L - 1 below)
  s[7] = 0.75                                                     # all scores tied: every OPA pair is wrong
  y[7, 0] = 2.0
  topn = max(L - 1, 1)
  desc = CUT_DESC(topn) + [(lm.ARP, None), (lm.OPA, None), (lm.MRR, None)]
  values, weights = _check(y, s, desc, f"L={L}")
  by = {NAMES[k]: m for m, (k, _) in enumerate(desc[:9])}
  assert not weights[:, 3].any() and not values[:, 3].any()
  for name in ("mrr", "hits", "precision", "recall", "map"):
    assert weights[by[name], 2] == 0.0 and weights[by[name], 5] == 0.0 and weights[by[name], 1] == 1.0
  assert values[by["mrr"], 1] == 1.0                               # (the cut L - 1 may drop the last of n = L items)
  assert values[by["map"], 1] >= 1.0 - 1.0 / L - 1e-6 and values[by["recall"], 1] >= 1.0 - 1.0 / L - 1e-6
  assert values[by["mrr"], 4] == 1.0 and values[by["precision"], 4] == np.float32(1.0) / np.float32(min(topn, L))
  assert weights[by["dcg"], 5] == 1.0 and weights[by["ndcg"], 5] == 1.0 and weights[by["dcg"], 2] == 0.0
  assert weights[by["arp"], 5] == 0.5 and values[by["opa"], 7] == 0.0
  if L >= 2:
    assert weights[by["opa"], 5] >= 1.0 and weights[by["opa"], 7] >= 1.0


def test_tied_scores_with_different_labels_count_against_opa():
  y = np.array([[1.0, 0.0, 2.0, -1.0, 0.0], [2.0, 1.0, 0.0, -1.0, -1.0]], dtype=np.float32)
  s = np.array([[0.5, 0.5, 0.9, 7.0, 0.5], [0.25, 0.25, 0.25, 0.0, 0.0]], dtype=np.float32)
  values, weights = _check(y, s, [(lm.OPA, None)], "ties")
  np.testing.assert_array_equal(weights[0], np.array([5.0, 3.0], dtype=np.float32))
  np.testing.assert_array_equal(values[0], np.array([np.float32(3.0) / np.float32(5.0), 0.0], dtype=np.float32))


# ---- 4. poisoned padding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 257])
def test_padded_scores_never_enter_the_arithmetic(L):
  B = 5
  y, s = lw.make_labels(B, L, 77 + L), lw.make_scores(B, L, 77 + L)
  y[0, L // 2] = -1.0
  pad = y < 0
  assert pad.any() and (~pad).any()
  desc = [(k, 3) for k in (lm.NDCG, lm.DCG, lm.MRR, lm.HITS, lm.PRECISION, lm.RECALL, lm.MAP)] + [(lm.ARP, None), (lm.OPA, None)]
  base = _call(y, s, desc)
  for poison in (np.nan, np.inf, -np.inf, 1e30):
    sp = s.copy()
    sp[pad] = poison
    got = _call(y, sp, desc)
    np.testing.assert_array_equal(_bits(got[0]), _bits(base[0]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(base[1]))


# ---- 5. group equals single ----------------------------------------------------------------------------------------------
GROUP16 = [(lm.NDCG, 10), (lm.NDCG, None), (lm.DCG, 10), (lm.DCG, 1), (lm.MRR, None), (lm.MRR, 10), (lm.HITS, 1),
           (lm.HITS, 10), (lm.PRECISION, 10), (lm.PRECISION, None), (lm.RECALL, 10), (lm.RECALL, 2000), (lm.MAP, None),
           (lm.MAP, 10), (lm.ARP, None), (lm.OPA, None)]


@pytest.mark.parametrize("B,L", [(67, 5), (67, 17), (67, 64), (67, 130), (3, 1024)])
def test_a_group_of_metrics_equals_the_one_metric_calls(B, L):
  """All nine kinds with several topns in one call of 16 descriptors, then 17 metrics through the Python function
  (two launches: the chunk edge): every row has the bits of the one-metric call, the NDCG rows those of
  ``tfrs_listwise_ndcg``."""
  from recommenders_amd import _lib, metrics
  y, s = _inputs(B, L, "half")
  values, weights = _call(y, s, GROUP16)
  singles = [_call(y, s, [d]) for d in GROUP16]
  for m, d in enumerate(GROUP16):
    np.testing.assert_array_equal(_bits(values[m]), _bits(singles[m][0][0]), err_msg=str(d))
    np.testing.assert_array_equal(_bits(weights[m]), _bits(singles[m][1][0]), err_msg=str(d))
  yt, st = _cuda(y), _cuda(s)
  for m, (kind, topn) in enumerate(GROUP16[:2]):
    out = torch.full((2, B), -7.0, device="cuda")
    _lib.check(_lib.load().tfrs_listwise_ndcg(_lib.ptr(yt), _lib.ptr(st), B, L, topn or 0, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                              _lib.current_stream()))
    np.testing.assert_array_equal(_bits(out[0]), _bits(values[m]))
    np.testing.assert_array_equal(_bits(out[1]), _bits(weights[m]))
  # 17 metrics: the per-list rows that update_listwise_metrics reduces (its chunk loop: two launches), bit for bit
  from recommenders_amd.metrics import listwise
  desc17 = GROUP16 + [(lm.MAP, 1)]
  rows = listwise._per_list(desc17, yt, st).cpu().numpy()
  assert rows.shape == (2, 17, B)
  for m, d in enumerate(desc17):
    v, w = singles[m] if m < 16 else _call(y, s, [d])
    np.testing.assert_array_equal(_bits(rows[0, m]), _bits(v[0]), err_msg=str(d))
    np.testing.assert_array_equal(_bits(rows[1, m]), _bits(w[0]), err_msg=str(d))
  # ... and through the function itself: each state is what the metric alone accumulates from the same per-list values
  # (the [B] sums are taken by torch on either route; compared to float32 rounding of a B-term sum)
  grouped = [_make(k, t) for k, t in desc17]
  alone = [_make(k, t) for k, t in desc17]
  metrics.update_listwise_metrics(grouped, yt, st)
  for g, a, (kind, topn) in zip(grouped, alone, desc17):
    a.update_state(yt, st)
    v, w = _call(y, s, [(kind, topn)])
    total, count = float(np.sum(v[0].astype(np.float64) * w[0])), float(np.sum(w[0].astype(np.float64)))
    for metric in (g, a):
      assert float(metric._count) == pytest.approx(count, rel=(B + 2) * lw.EPS), (kind, topn)
      assert float(metric._total) == pytest.approx(total, rel=(B + 2) * lw.EPS), (kind, topn)
  assert grouped[16]._group is grouped[0]._group and grouped[0]._group.state.shape == (3, 17)


# ---- 6. reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(67, 5), (67, 64), (67, 130), (3, 1024)])
def test_two_calls_give_identical_bits(B, L):
  y, s = _inputs(B, L, "graded")
  a, b = _call(y, s, GROUP16), _call(y, s, GROUP16)
  np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
  np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))


# ---- 7. update_state / result / reset_states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 5), (67, 9), (67, 33), (67, 130), (3, 1024)])
def test_results_over_two_updates(B, L):
  """Two updates, without a sample weight and with one ([B], then [B, 1]); every metric alone and all of them through
  ``update_listwise_metrics``: each result within the restatement's result bound; 0 after ``reset_states``."""
  from recommenders_amd import metrics
  seed = 900 * L + B
  batches = [(lm.make_half_labels(B, L, seed + k), lw.make_grid_scores(B, L, seed + k, step=0.5, lim=3.0)) for k in (0, 1)]
  weights = [(np.random.RandomState(seed + k).rand(B) + 0.25).astype(np.float32) for k in (0, 1)]
  desc = [(lm.NDCG, 10), (lm.DCG, 10), (lm.MRR, None), (lm.HITS, 1), (lm.PRECISION, 10), (lm.RECALL, 10), (lm.MAP, None),
          (lm.ARP, None), (lm.OPA, None)]
  for weighted in (False, True):
    updates = [(y, s, weights[k] if weighted else None) for k, (y, s) in enumerate(batches)]
    want = [lm.metric_result(kind, updates, topn) for kind, topn in desc]
    alone, grouped = [_make(k, t) for k, t in desc], [_make(k, t) for k, t in desc]
    assert all(float(m.result()) == 0.0 for m in alone + grouped)
    for k, (y, s, w) in enumerate(updates):
      wt = None if w is None else _cuda(w[:, None] if k else w)
      for m in alone:
        m.update_state(_cuda(y), _cuda(s), sample_weight=wt)
      metrics.update_listwise_metrics(grouped, _cuda(y), _cuda(s), sample_weight=wt)
    for (kind, topn), (value, bnd), a, g in zip(desc, want, alone, grouped):
      for route, m in (("alone", a), ("grouped", g)):
        got = float(m.result())
        print(f"{NAMES[kind]} topn={topn} {route} weighted={weighted}: {got!r} against {value!r}, bound {bnd:.3g}")
        assert abs(got - value) <= bnd + lw.FLOOR, (NAMES[kind], topn, route, weighted, got, value, bnd)
    for m in alone + grouped:
      m.reset_states()
      assert float(m.result()) == 0.0
    # the state survives the reset as storage: the next update starts from zero
    metrics.update_listwise_metrics(grouped, _cuda(batches[0][0]), _cuda(batches[0][1]))
    first = lm.metric_result(lm.MRR, [(batches[0][0], batches[0][1], None)])
    assert abs(float(grouped[2].result()) - first[0]) <= first[1] + lw.FLOOR


# ---- 8. captured step ----------------------------------------------------------------------------------------------------------
def test_captured_step_with_six_list_metrics_replays_the_eager_trajectory_bit_for_bit():
  import recommenders_amd as tfrs
  B, L = 48, 5

  class Ranker(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.items = tfrs.layers.embedding.Embedding(500, 16)
      self.score = tfrs.layers.blocks.Dense(1)
      m = tfrs.metrics
      self.list_metrics = [m.NDCGMetric(topn=3), m.MRRMetric(), m.MeanAveragePrecisionMetric(), m.PrecisionMetric(topn=3),
                           m.RecallMetric(topn=3), m.OPAMetric()]
      self.task = tfrs.tasks.Ranking(loss=tfrs.losses.PairwiseLogisticLoss(), metrics=self.list_metrics)

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
  assert all(float(m.result()) == 0.0 for m in graphed.list_metrics)
  start = [p.detach().clone() for p in eager.parameters()]
  names = [m.name for m in eager.list_metrics]
  assert names == ["ndcg_metric", "mrr_metric", "map_metric", "precision_metric", "recall_metric", "opa_metric"]
  for batch in batches:
    le, lg = eager.train_step(batch), step(batch)
    assert float(le["loss"]) == float(lg["loss"])
    for name in names:
      assert float(le[name]) == float(lg[name]), name
  for a, b, s0 in zip(eager.parameters(), graphed.parameters(), start):
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not torch.equal(a, s0)
  for me, mg in zip(eager.list_metrics, graphed.list_metrics):
    assert mg._group is graphed.list_metrics[0]._group and mg._group is not None       # one buffer, one launch
    for name in ("_total", "_count"):
      np.testing.assert_array_equal(_bits(getattr(me, name)), _bits(getattr(mg, name)))
    assert float(mg._count) > 0.0 and 0.0 < float(mg.result()) <= 1.0
  relevant = sum(int(((b["labels"] >= 1).sum(dim=1) > 0).sum()) for b in batches)
  assert float(eager.list_metrics[1]._count) == float(relevant)


# ---- 9. memory -----------------------------------------------------------------------------------------------------------------
def test_a_grouped_update_allocates_only_metric_by_list_sized_tensors():
  """B = 64, L = 1024, six metrics: the outputs are [2, M, B] floats; the update may add [M, B]-sized temporaries (a
  handful, each rounded up to the allocator's 512-byte granule) -- a [B, L] sort buffer would be 256 KiB, a
  [B, L, L] pair tensor 256 MiB."""
  from recommenders_amd import metrics
  B, L = 64, 1024
  yt, st = _cuda(lw.make_labels(B, L, 5)), _cuda(lw.make_scores(B, L, 5))
  ms = [_make(k, t) for k, t in ((lm.NDCG, 10), (lm.MRR, None), (lm.MAP, None), (lm.PRECISION, 10), (lm.RECALL, 10), (lm.OPA, None))]
  w = _cuda(lw.make_pow2_weights(B, 5))
  metrics.update_listwise_metrics(ms, yt, st, sample_weight=w)       # (library load, the shared state buffer)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  metrics.update_listwise_metrics(ms, yt, st, sample_weight=w)
  torch.cuda.synchronize()
  added = torch.cuda.max_memory_allocated() - before
  outputs = 2 * len(ms) * B * 4
  print(f"grouped update: peak over the inputs {added} bytes (outputs {outputs})")
  assert added <= outputs + 4 * (len(ms) * B * 4 + 512), added
  assert added < B * L * 4
  assert all(float(m._count) > 0.0 for m in ms)


# ---- 10. the C entry on the device box -----------------------------------------------------------------------------------------
def test_c_entry_validates_and_skips_empty_batches():
  from recommenders_amd import _lib, metrics
  lib = _lib.load()
  buf = torch.zeros(64, device="cuda")
  p, stream = _lib.ptr(buf), _lib.current_stream()
  null = ctypes.c_void_p(0)
  ints = lambda *v: (ctypes.c_int * len(v))(*v)
  calls = {
      "nmetrics 0": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 0, ints(0), ints(0), p, p, stream),
      "nmetrics 17": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 17, ints(*[0] * 17), ints(*[0] * 17), p, p, stream),
      "kind 9": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, ints(9), ints(0), p, p, stream),
      "topn -1": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, ints(lm.MAP), ints(-1), p, p, stream),
      "ARP topn": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, ints(lm.ARP), ints(2), p, p, stream),
      "OPA topn": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, ints(lm.OPA), ints(2), p, p, stream),
      "NULL labels": lambda: lib.tfrs_listwise_metrics(null, p, 2, 5, 1, ints(2), ints(0), p, p, stream),
      "NULL weights": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, ints(2), ints(0), p, null, stream),
      "NULL kinds": lambda: lib.tfrs_listwise_metrics(p, p, 2, 5, 1, None, ints(0), p, p, stream),
      "len 0": lambda: lib.tfrs_listwise_metrics(p, p, 2, 0, 1, ints(2), ints(0), p, p, stream),
      "len 1025": lambda: lib.tfrs_listwise_metrics(p, p, 2, 1025, 1, ints(2), ints(0), p, p, stream),
  }
  for what, call in calls.items():
    assert call() == _lib.TFRS_EINVAL, what
    assert "listwise_metrics" in _lib.last_error(), what
  assert lib.tfrs_listwise_metrics(null, null, 0, 5, 2, ints(lm.MRR, lm.OPA), ints(3, 0), null, null, stream) == _lib.TFRS_OK
  torch.cuda.synchronize()
  assert not buf.any()
  empty = torch.zeros(0, 5, device="cuda")
  ms = [metrics.MRRMetric(), metrics.OPAMetric(), metrics.DCGMetric(topn=2)]
  ms[0].update_state(empty, empty)
  metrics.update_listwise_metrics(ms, empty, empty)
  assert all(float(m.result()) == 0.0 for m in ms)
