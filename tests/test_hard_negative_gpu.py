"""Hard-negative mining and batch metrics over adjusted logits on the GPU (csrc/softmax_mined.hip): the selection
bit for bit on hand-built batches, loss and gradients against the float64 restatement on guarded random floats, the
kept set seen from both gradient kernels, rank counts, the routing of ``tasks.Retrieval``, peak memory, determinism
and graph capture.

Tolerances: the loss to 1e-5 relative (LOSS_RTOL, the project's loss tolerance); dq / dc through ``float_gate`` at
3.5e-6 of the sum of |terms| (GATE_SOFTMAX_GRAD["f32"]: the arithmetic per kept pair is the f32 softmax kernels').
Everything on hand-built inputs is compared with ``==``.  Observed on MI355X over every guarded case: loss 7.9e-8
relative, dq 1.9e-7, dc 4.8e-7 of the yardstick; the memory test peaks 18.7 MB above its inputs (limit 64 MB)."""

import contextlib

import numpy as np
import pytest

from oracle import retrieval as o_ret
from tests import hard_negative_handbuilt as hb
from tests import hard_negative_restatement as hn
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOSS_RTOL = 1e-5
GATE = 3.5e-6


def _t(a, **kw):
  return torch.as_tensor(np.asarray(a), **kw).cuda()


def _np(x):
  return x.detach().cpu().numpy()


@contextlib.contextmanager
def _waves(value):
  from recommenders_amd import _lib
  _lib.set_option("TFRS_SOFTMAX_WAVES", value)
  try:
    yield
  finally:
    _lib.set_option("TFRS_SOFTMAX_WAVES", None)


def _abi(case, weights=None, select=True, backward=False, count=False):
  """The C entry points on a hand-built case (the correction goes in as its log values): tau, cut, loss, dq, dc,
  counts as NumPy arrays."""
  from recommenders_amd import _lib
  lib = _lib.load()
  q, c = _t(case["q"]).contiguous(), _t(case["c"]).contiguous()
  (nq, d), nc = q.shape, c.shape[0]
  temp = 1.0 if case["temperature"] is None else float(case["temperature"])
  corr = None if case["log_corr"] is None else _t(case["log_corr"])
  ids = None if case["ids"] is None else _t(case["ids"]).long()
  mask = None if case["mask"] is None else _t(case["mask"]).to(torch.uint8).contiguous()
  w = None if weights is None else _t(np.asarray(weights, np.float32))
  ws = torch.empty((lib.tfrs_inbatch_mined_workspace_bytes(nq, nc, d),), dtype=torch.uint8, device="cuda")
  stream = _lib.current_stream()
  out = {}
  tau = cut = None
  if select and case["n"] is not None:
    tau = torch.full((nq,), float("nan"), device="cuda")
    cut = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.tfrs_inbatch_mined_select(_lib.ptr(q), _lib.ptr(c), nq, nc, d, temp, _lib.ptr(corr), _lib.ptr(ids),
                                             _lib.ptr(mask), int(case["n"]), _lib.ptr(tau), _lib.ptr(cut),
                                             _lib.ptr(ws), ws.numel(), stream))
    out.update(tau=_np(tau), cut=_np(cut))
  loss = torch.empty((), device="cuda")
  lse, pos = torch.empty((nq,), device="cuda"), torch.empty((nq,), device="cuda")
  _lib.check(lib.tfrs_inbatch_mined_ce_fwd(_lib.ptr(q), _lib.ptr(c), nq, nc, d, _lib.ptr(w), temp, _lib.ptr(corr),
                                           _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(tau), _lib.ptr(cut), _lib.ptr(loss),
                                           _lib.ptr(lse), _lib.ptr(pos), _lib.ptr(ws), ws.numel(), stream))
  out.update(loss=float(loss), pos=_np(pos))
  if backward:
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    _lib.check(lib.tfrs_inbatch_mined_ce_bwd(_lib.ptr(q), _lib.ptr(c), nq, nc, d, _lib.ptr(w), temp, _lib.ptr(corr),
                                             _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(tau), _lib.ptr(cut),
                                             _lib.ptr(lse), None, _lib.ptr(dq), _lib.ptr(dc), _lib.ptr(ws),
                                             ws.numel(), stream))
    out.update(dq=_np(dq), dc=_np(dc))
  if count:
    counts = torch.full((nq,), 12345, dtype=torch.int32, device="cuda")
    _lib.check(lib.tfrs_inbatch_mined_rank_count(_lib.ptr(q), _lib.ptr(c), nq, nc, d, temp, _lib.ptr(corr),
                                                 _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(tau), _lib.ptr(cut),
                                                 _lib.ptr(counts), _lib.ptr(ws), ws.numel(), stream))
    out.update(counts=_np(counts))
  return out


# ------------------------------------------------------------------------------------------ 1. the selection
@pytest.mark.parametrize("waves", [hb.GPU_TEST_WAVES, "1"])
@pytest.mark.parametrize("case", hb.selection_cases(), ids=lambda c: c["name"])
def test_selection_is_the_hand_built_expectation_bit_for_bit(case, waves):
  """tau as float32 bits, cut as int64, with every candidate tile a split of its own (the cut is then found across
  split boundaries) and with one split; the rank counts of the mined logits come with it."""
  exp = hb.expected(case)
  with _waves(waves):
    got = _abi(case, count=True)
  np.testing.assert_array_equal(got["tau"].view(np.uint32), exp["tau"].astype(np.float32).view(np.uint32))
  np.testing.assert_array_equal(got["cut"], exp["cut"])
  np.testing.assert_array_equal(got["counts"], exp["counts"])
  nq = case["q"].shape[0]
  np.testing.assert_array_equal(got["pos"].view(np.uint32), exp["s"][np.arange(nq), np.arange(nq)].view(np.uint32))
  assert got["loss"] == pytest.approx(hn.loss(exp["s"], exp["keep"]), rel=LOSS_RTOL, abs=1e-30)


def test_fully_masked_row_loses_log_of_its_kept_columns():
  case = hb.mask_case(5, None)
  for row, kept in ((7, 7), (9, 7)):
    got = _abi(case, weights=np.eye(40)[row])
    exp = hb.expected(case)
    assert got["loss"] == pytest.approx(hn.loss(exp["s"], exp["keep"], np.eye(40)[row]), rel=1e-6)
    if row == 7:
      assert got["loss"] == pytest.approx(np.log(float(kept)), rel=1e-6)


# ------------------------------------------------------------------------------------------ 2. loss and gradients
def _run_functional(q, c, n, kw, upstream=2.0):
  from recommenders_amd.tasks.retrieval import mined_in_batch_softmax_loss
  tq, tc = _t(q).requires_grad_(True), _t(c).requires_grad_(True)
  loss = mined_in_batch_softmax_loss(tq, tc, n, **{k: _t(v) if isinstance(v, np.ndarray) else v
                                                   for k, v in kw.items()})
  (loss * upstream).backward()
  return float(loss.detach()), _np(tq.grad) / upstream, _np(tc.grad) / upstream


_REFERENCE = {}


def _reference(shape, name, n):
  """Restatement values of a guarded case, computed once and shared."""
  key = (shape, name, n)
  if key not in _REFERENCE:
    q, c, variants = hn.guarded_case(*shape)
    kw = variants[name]
    s = hn.logits(q, c, **hn.logit_options(kw))
    keep = hn.kept_set(s, n)
    w, t, mask = kw.get("sample_weight"), kw.get("temperature"), kw.get("score_mask")
    _REFERENCE[key] = (hn.loss(s, keep, w),) + hn.loss_grads(q, c, s, keep, w, t, mask)
  return _REFERENCE[key]


@pytest.mark.parametrize("n", hn.GUARDED_NS)
@pytest.mark.parametrize("shape", hn.GUARDED_SHAPES, ids=str)
def test_loss_and_gradients_on_guarded_random_floats(shape, n):
  q, c, variants = hn.guarded_case(*shape)
  for name, kw in variants.items():
    ref, dq_ref, dc_ref, dq_y, dc_y = _reference(shape, name, n)
    loss, dq, dc = _run_functional(q, c, n, kw)
    err = abs(loss - ref) / max(abs(ref), 1e-30)
    eq = float_gate("softmax_mined.dq", dq, dq_ref, dq_y, GATE)
    ec = float_gate("softmax_mined.dc", dc, dc_ref, dc_y, GATE)
    print(f"{shape} n={n} {name}: loss rel err {err:.3e}, dq {eq:.3e}, dc {ec:.3e} (yardstick units)")
    assert err <= LOSS_RTOL, (name, loss, ref)


@pytest.mark.parametrize("shape", hn.GUARDED_SHAPES, ids=str)
def test_keeping_every_negative_is_the_in_batch_softmax(shape):
  from recommenders_amd.tasks.retrieval import in_batch_softmax_loss
  q, c, variants = hn.guarded_case(*shape)
  nc = shape[1]
  for name in ("plain", "all"):
    kw = {k: _t(v) if isinstance(v, np.ndarray) else v for k, v in variants[name].items()}
    want = float(in_batch_softmax_loss(_t(q), _t(c), **kw))
    for n in (nc - 1, nc + 10):
      got, _, _ = _run_functional(q, c, n, variants[name])
      assert got == pytest.approx(want, rel=LOSS_RTOL), (name, n)


# ------------------------------------------------------------------------------------------ 3. ties in the backward
@pytest.mark.parametrize("temperature,hits", [(None, True), (2.0, False)])
def test_both_gradient_kernels_keep_exactly_the_mined_set(temperature, hits):
  """The duplicated-row case, widened to 128 features that leave every logit as it is: features 16 .. 79 carry a
  one-hot code of the QUERY (zero in the candidates), features 80 .. 127 a one-hot code of 48 CANDIDATES at a time
  (zero in the queries).  Then dc[c, 16 + b] = G_bc and dq[b, 80 + k] = G_b,base+k, each a single term: the pair
  gradient as the dc kernel (queries streamed, operand roles swapped) and as the dq kernel formed it."""
  case = hb.duplicated_case(temperature, hits)
  exp = hb.expected(case)
  nq, nc, n = 64, 200, case["n"]
  p = hn.pair_gradient(exp["s"], exp["keep"], temperature=temperature)
  assert np.all(np.abs(p[exp["keep"]]) > 1e-30)                     # no kept probability underflows in float32
  g_dq = np.zeros((nq, nc), np.float32)
  g_dc = np.zeros((nq, nc), np.float32)
  for base in range(0, nc, 48):
    cols = np.arange(base, min(base + 48, nc))
    q = np.zeros((nq, 128), np.float32)
    c = np.zeros((nc, 128), np.float32)
    q[:, :16], c[:, :16] = case["q"], case["c"]
    q[np.arange(nq), 16 + np.arange(nq)] = 1.0
    c[cols, 80 + cols - base] = 1.0
    with _waves(hb.GPU_TEST_WAVES):
      got = _abi(dict(case, q=q, c=c), backward=True)
    np.testing.assert_array_equal(got["tau"].view(np.uint32), exp["tau"].view(np.uint32))
    np.testing.assert_array_equal(got["cut"], exp["cut"])
    g_dq[:, cols] = got["dq"][:, 80:80 + len(cols)]
    g_dc[:, cols] = got["dc"][cols, 16:16 + nq].T
    assert np.all(got["dc"][:, 16 + nq:80] == 0) and np.all(got["dq"][:, 16:80] == 0)
  for g in (g_dq, g_dc):
    np.testing.assert_array_equal(g != 0, exp["keep"])
    assert (g != 0).sum(axis=1).tolist() == [n + 1] * nq
    np.testing.assert_allclose(g, p, rtol=1e-4, atol=1e-30)
  np.testing.assert_array_equal(g_dq, g_dc)
  # dc of a copy is non-zero exactly where a row kept it
  plain = _abi(case, backward=True)
  np.testing.assert_array_equal(np.abs(plain["dc"][100:140]).sum(axis=1) != 0, exp["keep"][:, 100:140].any(axis=0))


# ------------------------------------------------------------------------------------------ 4. counts
def test_division_case_counts_and_hits():
  case = hb.division_case()
  got = _abi(case, count=True)
  assert got["counts"].tolist() == [0, 2]
  from recommenders_amd.tasks.retrieval import TopKCategoricalAccuracy
  metric = TopKCategoricalAccuracy(k=1)
  metric.update_from_adjusted(_t(case["q"]), _t(case["c"]), temperature=1.5)
  assert float(metric.result()) == 0.5


def _task_variants(v):
  """Constructor / call arguments of ``Retrieval`` for each adjustment of an ``option_variants`` dict."""
  call_all = dict(sample_weight=v["all"]["sample_weight"],
                  candidate_sampling_probability=v["all"]["candidate_sampling_probability"],
                  candidate_ids=v["all"]["candidate_ids"], score_mask=v["all"]["score_mask"])
  return {"temperature": (dict(temperature=0.7), dict()),
          "correction": (dict(), dict(candidate_sampling_probability=call_all["candidate_sampling_probability"])),
          "accidental_hits": (dict(remove_accidental_hits=True), dict(candidate_ids=call_all["candidate_ids"])),
          "mask": (dict(), dict(score_mask=call_all["score_mask"])),
          "mining": (dict(num_hard_negatives=7), dict()),
          "all": (dict(temperature=1.3, remove_accidental_hits=True, num_hard_negatives=7), call_all)}


def _metric_value(ctor, call, q, c, k, updates=1, explicit=False, monkeypatch=None):
  import recommenders_amd as tfrs
  from recommenders_amd.tasks.retrieval import TopKCategoricalAccuracy
  task = tfrs.tasks.Retrieval(batch_metrics=[TopKCategoricalAccuracy(k=k)], **ctor)
  with monkeypatch.context() as m:
    if explicit:
      m.setenv("TFRS_RETRIEVAL_EXPLICIT", "1")
    for _ in range(updates):
      task(_t(q), _t(c), compute_metrics=False, **{key: _t(val) for key, val in call.items()})
  return float(task.metrics[0].result())


@pytest.mark.parametrize("k", [1, 5])
def test_task_metric_equals_the_explicit_route_on_hand_built_inputs(k, monkeypatch):
  rng = np.random.default_rng(90)
  nq, nc, d = 40, 96, 12
  q = rng.integers(-3, 4, size=(nq, d)).astype(np.float32)
  c = rng.integers(-3, 4, size=(nc, d)).astype(np.float32)
  c[50:70] = c[0:20]                                                # copies of positives: exact ties
  for name, (ctor, call) in _task_variants(hn.option_variants(rng, nq, nc)).items():
    mined = _metric_value(ctor, call, q, c, k, monkeypatch=monkeypatch)
    explicit = _metric_value(ctor, call, q, c, k, explicit=True, monkeypatch=monkeypatch)
    assert mined == explicit, name


@pytest.mark.parametrize("k", [1, 5])
def test_task_metric_matches_the_oracle_on_guarded_random_inputs(k, monkeypatch):
  shape = hn.GUARDED_SHAPES[0]
  q, c, variants = hn.guarded_case(*shape)
  w = variants["all"]["sample_weight"]
  for name, (ctor, call) in _task_variants(variants).items():
    call = dict(call, sample_weight=w)
    okw = dict(temperature=ctor.get("temperature"), num_hard_negatives=ctor.get("num_hard_negatives"),
               candidate_sampling_probability=call.get("candidate_sampling_probability"),
               score_mask=call.get("score_mask"), candidate_ids=call.get("candidate_ids"),
               remove_accidental_hits_flag=bool(ctor.get("remove_accidental_hits")))
    s, labels = o_ret.logits_and_labels(q, c, **okw)
    hits = o_ret.batch_top_k_categorical_accuracy(labels, s, k)
    want = float((hits * w).sum() / w.sum())
    got = _metric_value(ctor, call, q, c, k, updates=2, monkeypatch=monkeypatch)
    assert got == pytest.approx(want, rel=1e-6), name


# ------------------------------------------------------------------------------------------ 5. routing
def _refuse(*args, **kwargs):
  raise AssertionError("the explicit score matrix was built")


def test_retrieval_routes_hard_negatives_and_adjusted_metrics_past_the_matrix(monkeypatch):
  import recommenders_amd as tfrs
  from recommenders_amd import _lib
  from recommenders_amd.tasks import retrieval as rt
  lib = _lib.load()
  rng = np.random.default_rng(31)
  nq, d = 64, 16
  w = rng.uniform(0.5, 2.0, size=nq).astype(np.float32)

  def configs():
    c_small = (rng.normal(size=(100, d)) / 2).astype(np.float32)
    c_wide = (rng.normal(size=(1500, d)) / 4).astype(np.float32)
    q = (rng.normal(size=(nq, d)) / 2).astype(np.float32)
    v = hn.option_variants(rng, nq, 100)["all"]
    return [
        (tfrs.tasks.Retrieval(num_hard_negatives=5, remove_accidental_hits=True, temperature=0.7), q, c_small,
         dict(candidate_ids=_t(v["candidate_ids"]), score_mask=_t(v["score_mask"]),
              candidate_sampling_probability=_t(v["candidate_sampling_probability"])),
         dict(num_hard_negatives=5, remove_accidental_hits_flag=True, temperature=0.7,
              candidate_ids=v["candidate_ids"], score_mask=v["score_mask"],
              candidate_sampling_probability=v["candidate_sampling_probability"])),
        (tfrs.tasks.Retrieval(batch_metrics=[rt.TopKCategoricalAccuracy(3)], temperature=0.5), q, c_small, dict(),
         dict(temperature=0.5)),
        (tfrs.tasks.Retrieval(num_hard_negatives=1200), q, c_wide, dict(), dict(num_hard_negatives=1200)),
    ]

  for task, q, c, call, okw in configs():
    with monkeypatch.context() as m:
      m.setattr(rt, "_DenseFn", type("NoDense", (), {"apply": staticmethod(_refuse)}))
      m.setattr(lib, "tfrs_compute_scores", _refuse)
      tq, tc = _t(q).requires_grad_(True), _t(c).requires_grad_(True)
      loss = task(tq, tc, sample_weight=_t(w), compute_metrics=False, **call)
      loss.backward()
      assert float(loss) == pytest.approx(float(o_ret.loss(q, c, sample_weight=w, **okw)), rel=LOSS_RTOL)
      assert float(tq.grad.abs().sum()) > 0 and float(tc.grad.abs().sum()) > 0
      # the switch restores the explicit route: the matrix is built again
      m.setenv("TFRS_RETRIEVAL_EXPLICIT", "1")
      with pytest.raises(AssertionError, match="explicit score matrix"):
        task(_t(q), _t(c), sample_weight=_t(w), compute_metrics=False, **call)


# ------------------------------------------------------------------------------------------ 6. memory
def test_peak_memory_stays_below_a_quarter_of_one_logits_matrix():
  from recommenders_amd.tasks.retrieval import mined_in_batch_softmax_loss
  nq, nc, d, n = 4096, 16384, 32, 50
  gen = torch.Generator(device="cuda").manual_seed(7)
  q = (torch.randn((nq, d), device="cuda", generator=gen) / d ** 0.25).requires_grad_(True)
  c = (torch.randn((nc, d), device="cuda", generator=gen) / d ** 0.25).requires_grad_(True)
  p = torch.rand((nc,), device="cuda", generator=gen)
  ids = torch.randint(0, nc // 2, (nc,), device="cuda", generator=gen)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  loss = mined_in_batch_softmax_loss(q, c, n, candidate_sampling_probability=p, candidate_ids=ids)
  loss.backward()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - before
  print(f"peak above the inputs: {peak / 2 ** 20:.1f} MB")
  assert peak < nq * nc * 4 // 4
  assert np.isfinite(float(loss)) and float(q.grad.abs().sum()) > 0 and float(c.grad.abs().sum()) > 0


# ------------------------------------------------------------------------------------------ 7. determinism, capture
def _mined_step(q, c, kw, n):
  from recommenders_amd.tasks.retrieval import mined_in_batch_softmax_loss
  q.grad = c.grad = None
  loss = mined_in_batch_softmax_loss(q, c, n, **kw)
  loss.backward()
  return loss


def test_two_eager_runs_and_a_graph_replay_give_identical_bits():
  shape = hn.GUARDED_SHAPES[0]
  qn, cn, variants = hn.guarded_case(*shape)
  kw = {k: _t(v) if isinstance(v, np.ndarray) else v for k, v in variants["all"].items()}
  q, c = _t(qn).requires_grad_(True), _t(cn).requires_grad_(True)
  runs = []
  for _ in range(2):
    loss = _mined_step(q, c, kw, 7)
    runs.append((_np(loss).copy(), _np(q.grad).copy(), _np(c.grad).copy()))
  for a, b in zip(*runs):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
  # capture forward + backward on one stream and replay
  sq, sc = q.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      _mined_step(sq, sc, kw, 7)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  sq.grad = sc.grad = None
  with torch.cuda.graph(graph):
    from recommenders_amd.tasks.retrieval import mined_in_batch_softmax_loss
    gl = mined_in_batch_softmax_loss(sq, sc, 7, **kw)
    gl.backward()
  for _ in range(2):
    sq.grad.zero_()
    sc.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(runs[0], (_np(gl), _np(sq.grad), _np(sc.grad))):
      np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_captured_train_step_replays_the_mined_route():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(3)
  d = 32

  class TwoTower(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.user_model = tfrs.layers.embedding.Embedding(943, d)
      self.item_model = tfrs.layers.embedding.Embedding(1682, d)
      self.task = tfrs.tasks.Retrieval(temperature=0.5, num_hard_negatives=20, remove_accidental_hits=True)

    def compute_loss(self, features, training=False):
      return self.task(self.user_model(features["user_id"]), self.item_model(features["movie_id"]),
                       candidate_ids=features["movie_id"], compute_metrics=False)

  def make():
    torch.manual_seed(5)
    m = TwoTower()
    m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.5))
    return m

  batches = [{"user_id": _t(rng.integers(0, 943, size=300)),
              "movie_id": _t(rng.integers(0, 1682, size=300))} for _ in range(3)]
  eager, graphed = make(), make()
  step = graphed.make_graphed_train_step(batches[0])
  for batch in batches:
    le = eager.train_step(batch)
    lg = step(batch)
    assert float(le["loss"]) == float(lg["loss"])
  for a, b in zip(eager.parameters(), graphed.parameters()):
    np.testing.assert_array_equal(_np(a), _np(b))
