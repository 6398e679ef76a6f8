"""The list metrics of DESIGN 4.26 without a GPU: the restatement (tests/listwise_metrics_restatement.py) against lists
worked by hand, its padding behaviour, the exactness argument behind the bit-equal GPU tests, and the host-side
validation of the product classes and of ``tfrs_listwise_metrics`` (which rejects bad arguments before any device
call)."""

import math

import numpy as np
import pytest
import torch

from tests import listwise_metrics_restatement as lm

CUT_KINDS = (lm.MRR, lm.HITS, lm.PRECISION, lm.RECALL, lm.MAP, lm.DCG)
ALL_KINDS = CUT_KINDS + lm.UNCUT_KINDS


def _v(kind, y, s, topn=None):
  m = lm.list_metric(kind, y, s, topn)
  return m.value, m.weight


# ---- by hand -----------------------------------------------------------------------------------------------------------
# labels (0, 1, 0, 2, 1), scores rank the positions 2, 1, 4, 0, 3: rel in rank order 0 1 1 0 1, c = 0 1 2 2 3, R = 3
Y5, S5 = [0.0, 1.0, 0.0, 2.0, 1.0], [0.2, 0.8, 0.9, 0.1, 0.5]


def test_each_metric_by_hand():
  assert lm.score_order(Y5, S5) == [2, 1, 4, 0, 3]
  assert _v(lm.MRR, Y5, S5) == (0.5, 1.0) and _v(lm.MRR, Y5, S5, 1) == (0.0, 1.0) and _v(lm.MRR, Y5, S5, 2) == (0.5, 1.0)
  assert _v(lm.HITS, Y5, S5) == (1.0, 1.0) and _v(lm.HITS, Y5, S5, 1) == (0.0, 1.0)
  assert _v(lm.PRECISION, Y5, S5) == (3.0 / 5.0, 1.0)                      # topn None: the padded width
  assert _v(lm.PRECISION, Y5, S5, 3) == (2.0 / 3.0, 1.0) and _v(lm.PRECISION, Y5, S5, 2000) == (3.0 / 5.0, 1.0)
  assert _v(lm.RECALL, Y5, S5) == (1.0, 1.0) and _v(lm.RECALL, Y5, S5, 3) == (2.0 / 3.0, 1.0)
  assert _v(lm.MAP, Y5, S5)[0] == pytest.approx((1.0 / 2.0 + 2.0 / 3.0 + 3.0 / 5.0) / 3.0, rel=1e-15)
  assert _v(lm.MAP, Y5, S5, 3)[0] == pytest.approx((1.0 / 2.0 + 2.0 / 3.0) / 3.0, rel=1e-15)
  dcg = 0.0 + 1.0 / math.log2(3.0) + 1.0 / 2.0 + 0.0 + 3.0 / math.log2(6.0)
  assert _v(lm.DCG, Y5, S5)[0] == pytest.approx(dcg, rel=1e-15) and _v(lm.DCG, Y5, S5)[1] == 1.0
  assert _v(lm.DCG, Y5, S5, 2)[0] == pytest.approx(1.0 / math.log2(3.0), rel=1e-15)
  # ARP: sum y (r + 1) = 1 * 2 + 1 * 3 + 2 * 5 = 15 over sum y = 4
  assert _v(lm.ARP, Y5, S5) == (15.0 / 4.0, 4.0)
  # OPA: P = 2 * 2 (a 1 over a 0) + 2 (the 2 over the 0s) + 2 (the 2 over the 1s) = 8; the item labelled 2 ranks last
  # and wins nothing; item 1 (0.8) beats position 0 only, item 4 (0.5) beats position 0 only: C = 2
  m = lm.list_metric(lm.OPA, Y5, S5)
  assert (m.num, m.den, m.value, m.weight) == (2, 8, 0.25, 8.0)


def test_integer_metrics_carry_their_integers():
  for kind, topn, num, den in ((lm.MRR, None, 1, 2), (lm.MRR, 1, 0, 1), (lm.HITS, 2, 1, 1), (lm.PRECISION, 3, 2, 3),
                               (lm.PRECISION, None, 3, 5), (lm.RECALL, 3, 2, 3), (lm.RECALL, 1, 0, 3)):
    m = lm.list_metric(kind, Y5, S5, topn)
    assert (m.num, m.den) == (num, den), (kind, topn)
    assert m.value == num / den


def test_ties_and_cuts():
  # tied scores keep the position order: the relevant item at the later position falls outside a cut between them
  assert _v(lm.HITS, [0.0, 1.0], [0.5, 0.5], 1) == (0.0, 1.0) and _v(lm.HITS, [1.0, 0.0], [0.5, 0.5], 1) == (1.0, 1.0)
  assert _v(lm.MRR, [0.0, 1.0], [0.5, 0.5]) == (0.5, 1.0)
  # tied scores with different labels count against OPA
  m = lm.list_metric(lm.OPA, [1.0, 0.0, 2.0], [0.5, 0.5, 0.9])
  assert (m.num, m.den) == (2, 3)
  # n < topn: the cut is n
  assert _v(lm.RECALL, [1.0, -1.0, 0.0, -1.0], [0.1, 9.0, 0.2, 9.0], 3) == (1.0, 1.0)
  assert _v(lm.PRECISION, [1.0, -1.0, 0.0, -1.0], [0.1, 9.0, 0.2, 9.0], 3) == (1.0 / 3.0, 1.0)


def test_lists_that_do_not_count():
  for kind in ALL_KINDS:
    assert _v(kind, [-1.0, -1.0], [1.0, 2.0]) == (0.0, 0.0), kind                    # all padding
    assert _v(kind, [0.0, 0.0, -1.0], [1.0, 2.0, 3.0]) == (0.0, 0.0), kind           # nothing relevant, no gain
  # a label of 0.5 is not relevant, but it has gain, relevance mass and pairs
  y, s = [0.5, 0.0, -1.0], [0.1, 0.9, 0.5]
  for kind in (lm.MRR, lm.HITS, lm.PRECISION, lm.RECALL, lm.MAP):
    assert _v(kind, y, s) == (0.0, 0.0), kind
  assert _v(lm.DCG, y, s)[1] == 1.0 and _v(lm.DCG, y, s)[0] == pytest.approx((2.0 ** 0.5 - 1.0) / math.log2(3.0), rel=1e-15)
  assert _v(lm.ARP, y, s) == (2.0, 0.5)
  assert _v(lm.OPA, y, s) == (0.0, 1.0)
  # one valid item; all items relevant
  assert _v(lm.MRR, [-1.0, 3.0, -1.0], [0.0, 0.0, 0.0]) == (1.0, 1.0) and _v(lm.OPA, [-1.0, 3.0, -1.0], [0.0] * 3) == (0.0, 0.0)
  assert _v(lm.MAP, [1.0, 2.0, 1.0], [0.3, 0.2, 0.1]) == (1.0, 1.0) and _v(lm.PRECISION, [1.0, 2.0, 1.0], [0.3, 0.2, 0.1], 2) == (1.0, 1.0)


def test_result_is_the_weighted_mean_and_pools_arp_and_opa():
  y = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, -1.0]])
  s = np.array([[1.0, 2.0, 3.0], [0.9, 0.1, 0.5], [0.9, 0.1, 0.5]])
  assert lm.metric_result(lm.MRR, [(y, s, None)])[0] == pytest.approx((1.0 / 3.0 + 1.0) / 2.0, rel=1e-15)      # list 0 does not count
  assert lm.metric_result(lm.MRR, [(y, s, [5.0, 1.0, 3.0])])[0] == pytest.approx((1.0 / 3.0 + 3.0) / 4.0, rel=1e-15)
  assert lm.metric_result(lm.MRR, [(y[:1], s[:1], None)]) == (0.0, 0.0)
  # OPA pools the pairs: (0 + 1) right of (2 + 1) pairs; ARP pools the relevance mass: (3 + 1) / 2
  assert lm.metric_result(lm.OPA, [(y, s, None)])[0] == pytest.approx(1.0 / 3.0, rel=1e-15)
  assert lm.metric_result(lm.ARP, [(y, s, None)])[0] == pytest.approx(2.0, rel=1e-15)
  two = lm.metric_result(lm.OPA, [(y[1:2], s[1:2], None), (y[2:], s[2:], [2.0])])
  assert two[0] == pytest.approx((0.0 + 2.0) / (2.0 + 2.0), rel=1e-15) and 0.0 < two[1] < 1e-5


# ---- padding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_moving_or_adding_padding_changes_only_what_the_formulas_say(kind):
  """Only ``PrecisionMetric`` without a cut depends on the padded width (its denominator is L by definition)."""
  for topn in ((None,) if kind in lm.UNCUT_KINDS else (None, 2, 4)):
    base = lm.list_metric(kind, Y5, S5, topn)
    for at in range(len(Y5) + 1):
      for pads in (1, 3):
        yp = Y5[:at] + [-1.0] * pads + Y5[at:]
        sp = S5[:at] + [123.0] * pads + S5[at:]
        got = lm.list_metric(kind, yp, sp, topn)
        assert got.weight == base.weight
        if kind == lm.PRECISION and (topn is None or topn > len(Y5)):
          assert got.num == base.num and got.den == len(yp)
        else:
          assert got.value == pytest.approx(base.value, rel=1e-15)
          assert (got.num, got.den) == (base.num, base.den)


# ---- exactness of the bit-equal GPU tests ------------------------------------------------------------------------------
def test_integers_of_the_bit_equal_tests_are_exact_in_float32():
  """A numerator or denominator is at most L^2 = 2^20 < 2^24 (``BatchMetric`` asserts it for every batch it is given), so
  both convert to float32 exactly, and the correctly rounded float32 quotient of two exact operands IS the float64
  quotient rounded once."""
  assert lm.lw.MAX_LIST_LEN ** 2 < 2 ** 24
  for B, L in ((3, 5), (3, 130), (1, 1024)):
    y, s = lm.make_labels(B, L, 31 + L), lm.make_grid_scores(B, L, 31 + L)
    for kind in lm.INTEGER_KINDS:
      m = lm.BatchMetric(kind, y, s, None if kind in lm.UNCUT_KINDS else 10)
      np.testing.assert_array_equal(m.f32, (m.num / m.den).astype(np.float32))
      np.testing.assert_array_equal(m.weight.astype(np.float32).astype(np.float64), m.weight)


def test_input_makers():
  y = lm.make_sparse_binary_labels(67, 33, 9)
  assert set(np.unique(y)) == {-1.0, 0.0, 1.0}
  relevant = (y >= 1.0).sum(axis=1)
  assert (relevant == 0).any() and (relevant == 1).sum() > 30 and relevant.max() <= 2
  h = lm.make_half_labels(67, 33, 9)
  assert (h == 0.5).any() and not (h == 4.0).any() and (h == -1.0).any()


# ---- validation --------------------------------------------------------------------------------------------------------
def _cut_classes():
  from recommenders_amd import metrics
  return {"mrr_metric": metrics.MRRMetric, "hits_metric": metrics.HitsMetric, "precision_metric": metrics.PrecisionMetric,
          "recall_metric": metrics.RecallMetric, "map_metric": metrics.MeanAveragePrecisionMetric,
          "dcg_metric": metrics.DCGMetric, "ndcg_metric": metrics.NDCGMetric}


def test_constructors_and_shapes_are_validated_before_the_device():
  from recommenders_amd import metrics
  y, s = torch.zeros(4, 5), torch.zeros(4, 5)
  made = []
  for name, cls in _cut_classes().items():
    assert cls().name == name and cls().topn is None and cls("x", 7).topn == 7 and cls(topn=3).name == name
    for bad in (0, -3, 2.5):
      with pytest.raises(ValueError, match=f"{cls.__name__}: topn"):
        cls(topn=bad)
    made.append(cls(topn=5))
  for name, cls in (("arp_metric", metrics.ARPMetric), ("opa_metric", metrics.OPAMetric)):
    assert cls().name == name and cls("x").name == "x" and cls().topn is None
    with pytest.raises(TypeError):
      cls(topn=3)
    made.append(cls())
  for m in made:
    with pytest.raises(ValueError, match="per list"):
      m.update_state(y, s, sample_weight=torch.ones(4, 5))
    with pytest.raises(ValueError, match=r"\[batch, list\]"):
      m.update_state(torch.zeros(5), torch.zeros(5))
    with pytest.raises(ValueError, match="MAX_LIST_LEN"):
      m.update_state(torch.zeros(2, 1025), torch.zeros(2, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      m.update_state(y, s)
    assert float(m.result()) == 0.0
    m.reset_states()
  # the grouped update: the same checks, once for all
  with pytest.raises(ValueError, match="per list"):
    metrics.update_listwise_metrics(made, y, s, sample_weight=torch.ones(4, 5))
  with pytest.raises(ValueError, match="MAX_LIST_LEN"):
    metrics.update_listwise_metrics(made, torch.zeros(2, 1025), torch.zeros(2, 1025))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    metrics.update_listwise_metrics(made, y, s)
  with pytest.raises(TypeError, match="not a listwise metric"):
    metrics.update_listwise_metrics([made[0], metrics.Mean()], y, s)
  with pytest.raises(ValueError, match="twice"):
    metrics.update_listwise_metrics([made[0], made[0]], y, s)
  metrics.update_listwise_metrics([], y, s)
  assert all(float(m.result()) == 0.0 for m in made)


def test_a_ranking_task_groups_two_or_more_list_metrics_only(monkeypatch):
  """One list metric, or none, takes the path it always took; two or more go through ``update_listwise_metrics`` and the
  other metrics are still updated one by one."""
  from recommenders_amd import metrics, tasks
  from recommenders_amd.metrics import listwise
  calls = []
  monkeypatch.setattr(listwise, "update_listwise_metrics", lambda ms, *a, **k: calls.append(("group", list(ms))))
  for cls in (metrics.NDCGMetric, metrics.MRRMetric, metrics.OPAMetric, metrics.RootMeanSquaredError):
    monkeypatch.setattr(cls, "update_state", lambda self, *a, **k: calls.append(("single", self)))
  loss = lambda y_true, y_pred, sample_weight=None: torch.zeros(())
  y = torch.zeros(2, 3)
  ndcg, mrr, opa, rmse = metrics.NDCGMetric(), metrics.MRRMetric(), metrics.OPAMetric(), metrics.RootMeanSquaredError()
  tasks.Ranking(loss=loss, metrics=[rmse, ndcg])(y, y)
  assert calls == [("single", rmse), ("single", ndcg)]
  del calls[:]
  tasks.Ranking(loss=loss, metrics=[ndcg, rmse, mrr, opa])(y, y)
  assert calls == [("group", [ndcg, mrr, opa]), ("single", rmse)]


def test_c_entry_rejects_bad_arguments_before_any_device_call():
  import ctypes
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  lib = _lib.load()
  p = ctypes.c_void_p(256)       # never dereferenced: every call below returns before a launch
  ints = lambda *v: (ctypes.c_int * len(v))(*v)

  def call(kinds=(lm.MRR,), topns=(0,), n=None, y=p, s=p, nlists=2, length=5, values=p, weights=p):
    return lib.tfrs_listwise_metrics(y, s, nlists, length, len(kinds) if n is None else n,
                                     ints(*kinds) if kinds is not None else None,
                                     ints(*topns) if topns is not None else None, values, weights, None)

  bad = {
      "nmetrics 0": (lambda: call(n=0), "nmetrics"), "nmetrics 17": (lambda: call((0,) * 17, (0,) * 17), "nmetrics"),
      "nmetrics -1": (lambda: call(n=-1), "nmetrics"),
      "kind 9": (lambda: call((lm.MRR, 9), (0, 0)), "unknown kind"), "kind -1": (lambda: call((-1,)), "unknown kind"),
      "topn -1": (lambda: call((lm.NDCG, lm.MAP), (3, -1)), "topn"),
      "ARP topn": (lambda: call((lm.ARP,), (3,)), "ARP and OPA"), "OPA topn": (lambda: call((lm.MRR, lm.OPA), (3, 1)), "ARP and OPA"),
      "NULL kinds": (lambda: call(None, (0,), n=1), "NULL"), "NULL topns": (lambda: call((0,), None, n=1), "NULL"),
      "NULL labels": (lambda: call(y=None), "NULL pointer"), "NULL scores": (lambda: call(s=None), "NULL pointer"),
      "NULL values": (lambda: call(values=None), "NULL pointer"), "NULL weights": (lambda: call(weights=None), "NULL pointer"),
      "len 0": (lambda: call(length=0), "len"), "len 1025": (lambda: call(length=1025), "len"),
      "nlists < 0": (lambda: call(nlists=-1), "nlists"), "2^31": (lambda: call(nlists=2 ** 31 // 1024, length=1024), "2^31"),
  }
  for what, (fn, text) in bad.items():
    rc = fn()
    assert rc == _lib.TFRS_EINVAL and "listwise_metrics" in _lib.last_error() and text in _lib.last_error(), (
        what, rc, _lib.last_error())
  # every kind with a legal topn passes the checks; with no lists that is all there is to do (no device here)
  assert call(tuple(range(9)), (1, 0, 5, 2 ** 31 - 1, 0, 7, 0, 0, 0), nlists=0, y=None, s=None, values=None,
              weights=None) == _lib.TFRS_OK
  assert call((lm.OPA,) * 16, (0,) * 16, nlists=0) == _lib.TFRS_OK
  # the NDCG entry keeps its own validation and messages
  assert lib.tfrs_listwise_ndcg(p, p, 2, 5, -1, p, p, None) == _lib.TFRS_EINVAL and "listwise_ndcg: topn" in _lib.last_error()
  assert lib.tfrs_listwise_ndcg(None, None, 0, 5, 3, None, None, None) == _lib.TFRS_OK


def test_the_metrics_kernel_uses_no_scratch_and_the_ndcg_kernel_is_gone():
  """From the code object metadata of the cross-compiled source: five instantiations, no private segment, no spills,
  LDS no larger than the file's other kernels take (8 KiB below G = 256, 32 KiB there, + the four reduction words)."""
  import os
  import re
  import subprocess
  import tempfile
  from recommenders_amd.csrc import build as csrc_build
  src = os.path.join(os.path.dirname(csrc_build.__file__), "listwise.hip")
  out = os.path.join(tempfile.mkdtemp(prefix="tfrs_listwise_metrics_"), "listwise.s")
  subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17",
                  *csrc_build.EXTRA_FLAGS.get("listwise.hip", []), "-S", "--cuda-device-only", "-o", out, src],
                 check=True, capture_output=True, cwd=os.path.dirname(src))
  with open(out) as f:
    asm = f.read()
  lds = {}
  for block in asm.split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", block).group(1)
    assert "listwise_ndcg_kernel" not in name
    if "listwise_metrics_kernel" not in name:
      continue
    g = int(re.search(r"listwise_metrics_kernelILi(\d+)E", name).group(1))
    lds[g] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  assert lds == {8: 8192 + 16, 16: 8192 + 16, 32: 8192 + 16, 64: 8192 + 16, 256: 32768 + 16}
