"""Mined in-batch softmax without a GPU: the restatement the GPU tests compare against (the oracle's loss and kept
columns, the guard on every random case, the ties the hand-built cases claim), the new C entry points (header,
library, binding, argument checks before the device is touched) and the split plans the GPU tests rely on."""

import ctypes
import os
import re

import numpy as np
import pytest

from oracle import retrieval as o_ret
from tests import hard_negative_handbuilt as hb
from tests import hard_negative_restatement as hn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tfrs_inbatch_mined_workspace_bytes", "tfrs_inbatch_mined_plan", "tfrs_inbatch_mined_select",
               "tfrs_inbatch_mined_ce_fwd", "tfrs_inbatch_mined_ce_bwd", "tfrs_inbatch_mined_rank_count")


# ------------------------------------------------------------------------------------------ the restatement
def _oracle_kw(kw, n):
  okw = {k: v for k, v in kw.items() if k != "candidate_ids"}
  if "candidate_ids" in kw:
    okw.update(candidate_ids=kw["candidate_ids"], remove_accidental_hits_flag=True)
  return dict(okw, num_hard_negatives=n)


@pytest.mark.parametrize("n", [0, 1, 5, 36, 60])
def test_restatement_loss_and_kept_columns_are_the_oracle_s(n):
  """Every option combination.  The oracle forms its logits in float32; the restatement is given the same float32
  logits here, so the kept columns agree exactly and the losses to 1e-12 (both sum in float64)."""
  rng = np.random.default_rng(5)
  nq, nc, d = 23, 37, 12
  q = rng.normal(size=(nq, d)).astype(np.float32)
  c = rng.normal(size=(nc, d)).astype(np.float32)
  for name, kw in hn.option_variants(rng, nq, nc).items():
    okw = _oracle_kw(kw, n)
    s, _ = o_ret.logits_and_labels(q, c, **{k: v for k, v in okw.items()
                                            if k not in ("sample_weight", "num_hard_negatives")})
    want_logits, want_labels = o_ret.hard_negative_mining(s, np.eye(nq, nc, dtype=np.float32), n)
    cols = hn.kept_columns(s, n)
    np.testing.assert_array_equal(np.take_along_axis(s, cols, 1), want_logits, err_msg=name)
    np.testing.assert_array_equal(cols[:, 0], np.arange(nq))
    keep = hn.kept_set(s, n)
    assert keep.sum(axis=1).tolist() == [min(n, nc - 1) + 1] * nq
    np.testing.assert_array_equal(hn.keep_from_tau_cut(s, *hn.tau_cut(s, n)), keep)
    z = want_logits.astype(np.float64)
    z = z - z.max(axis=1, keepdims=True)
    per_row = -(want_labels * (z - np.log(np.exp(z).sum(axis=1, keepdims=True)))).sum(axis=1)
    if "sample_weight" in kw:
      per_row = per_row * kw["sample_weight"].astype(np.float64)
    assert hn.loss(s, keep, kw.get("sample_weight")) == pytest.approx(float(per_row.sum()), rel=1e-12), name
    # oracle.retrieval.loss itself returns that sum rounded to float32
    assert float(np.float32(hn.loss(s, keep, kw.get("sample_weight")))) == pytest.approx(
        float(o_ret.loss(q, c, **okw)), rel=1e-12), name
    # ... and the float64 logits of the restatement give the same loss up to the float32 rounding of the oracle's
    s64 = hn.logits(q, c, **hn.logit_options(kw))
    assert hn.loss(s64, hn.kept_set(s64, n), kw.get("sample_weight")) == pytest.approx(float(per_row.sum()), rel=1e-5)


def test_restatement_gradients_agree_with_central_differences():
  rng = np.random.default_rng(11)
  nq, nc, d, n = 5, 9, 4, 3
  q = rng.normal(size=(nq, d))
  c = rng.normal(size=(nc, d))
  for name, kw in hn.option_variants(rng, nq, nc).items():
    lkw = hn.logit_options(kw)
    w, t, mask = kw.get("sample_weight"), kw.get("temperature"), kw.get("score_mask")
    s = hn.logits(q, c, **lkw)
    gap, _ = hn.boundary_gap_guard(q, c, s, n, t)
    if gap.min() < 1e-3:
      continue                                           # the kept set must not change inside the difference stencil
    keep = hn.kept_set(s, n)
    dq, dc, _, _ = hn.loss_grads(q, c, s, keep, w, t, mask)
    eps = 1e-6
    for arr, grad in ((q, dq), (c, dc)):
      num = np.zeros_like(arr)
      it = np.nditer(arr, flags=["multi_index"])
      for _ in it:
        i = it.multi_index
        old = arr[i]
        arr[i] = old + eps
        up = hn.loss(hn.logits(q, c, **lkw), keep, w)
        arr[i] = old - eps
        down = hn.loss(hn.logits(q, c, **lkw), keep, w)
        arr[i] = old
        num[i] = (up - down) / (2 * eps)
      np.testing.assert_allclose(grad, num, rtol=1e-5, atol=1e-7, err_msg=name)


@pytest.mark.parametrize("shape", hn.GUARDED_SHAPES, ids=str)
def test_every_row_of_every_random_case_passes_the_guard(shape):
  q, c, variants = hn.guarded_case(*shape)
  assert q.shape == shape[::2] and np.isfinite(q).all()
  for name, kw in variants.items():
    s = hn.logits(q, c, **hn.logit_options(kw))
    for n in hn.GUARDED_NS:
      gap, bound = hn.boundary_gap_guard(q, c, s, n, kw.get("temperature"))
      assert gap.shape == (shape[0],) and bound > 0
      assert (gap > bound).all(), (name, n, float(gap.min()), bound)


def test_hand_built_cases_contain_the_ties_they_claim():
  cases = hb.selection_cases()
  assert {(c["q"].shape[0], c["c"].shape[0], c["q"].shape[1]) for c in cases} == {
      (5, 7, 3), (33, 70, 8), (64, 200, 16), (40, 96, 5), (40, 96, 100)}
  assert {c["n"] for c in cases if c["q"].shape[0] == 5} == {0, 1, 3, 5, 6, 50}
  assert {c["temperature"] for c in cases} == set(hb.TEMPERATURES)
  with_cut = 0
  for case in cases:
    exp = hb.expected(case)
    for arr in (case["q"], case["c"]):
      assert np.array_equal(arr, np.round(arr)) and np.abs(arr).max() <= 3
    if case["log_corr"] is not None:
      assert np.array_equal(case["log_corr"] * 8, np.round(case["log_corr"] * 8))
    np.testing.assert_array_equal(hn.keep_from_tau_cut(exp["s"], exp["tau"], exp["cut"]), exp["keep"])
    for row, cut in case["planted"]:
      assert exp["cut"][row] == cut, (case["name"], row)
    with_cut += int(((exp["cut"] >= 0) & (exp["cut"] != hn.CUT_ALL)).sum())
    if case["n"] == 0:
      assert np.all(np.isposinf(exp["tau"])) and np.all(exp["cut"] == -1)
  assert with_cut > 100
  # the copies tie: five tiles apart, and as accidental hits they are MIN_FLOAT exactly
  dup = hb.duplicated_case(1.5, True)
  s = hb.expected(dup)["s"]
  rows = np.arange(40)
  assert np.all(s[rows, 100 + rows] == hn.MIN_FLOAT)
  free = hb.expected(hb.duplicated_case(None, False))["s"]
  np.testing.assert_array_equal(free[:, 100:140], free[:, 0:40])
  # the masked rows
  m = hb.expected(hb.mask_case(5, None))
  assert np.all(m["s"][7] == hn.MIN_FLOAT) and m["keep"][7].sum() == 7
  assert hn.loss(m["s"], m["keep"], np.eye(40)[7]) == pytest.approx(np.log(7.0), rel=1e-12)
  assert (m["s"][9] > hn.MIN_FLOAT).sum() == 3


def test_division_case_needs_the_division():
  case = hb.division_case()
  exp = hb.expected(case)
  assert exp["s"][0, 0] == exp["s"][0, 2] == np.float32(8388609.0)
  assert exp["counts"].tolist() == [0, 2] and hn.top_k_hits(exp["s"], exp["keep"], 1).tolist() == [1.0, 0.0]
  inv = np.float32(1.0) / np.float32(1.5)
  dots = (case["q"].astype(np.float64) @ case["c"].astype(np.float64).T).astype(np.float32)
  assert (dots[0, 0], dots[0, 2]) == (12582913.0, 12582914.0)
  assert (dots[0, 0] * inv, dots[0, 2] * inv) == (np.float32(8388609.0), np.float32(8388610.0))


# ------------------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


def test_new_symbols_are_in_the_header_the_library_and_the_binding(lib):
  from recommenders_amd import _lib
  from recommenders_amd.csrc import build as csrc_build
  from recommenders_amd.tasks import retrieval as rt
  with open(os.path.join(ROOT, "include", "tfrs_hip.h")) as f:
    header = f.read()
  for name in NEW_SYMBOLS:
    assert re.search(r"\b%s\(" % name, header), name
    assert hasattr(lib, name), name
    assert name in _lib.SIGNATURES, name
  assert "softmax_mined.hip" in csrc_build.SOURCES
  assert callable(rt.mined_in_batch_softmax_loss) and hasattr(rt.TopKCategoricalAccuracy, "update_from_adjusted")


_BUF = ctypes.create_string_buffer(64)            # a non-NULL host address: never dereferenced by a refused call
_PTR = ctypes.c_void_p(ctypes.addressof(_BUF))
_DEFAULTS = dict(q=_PTR, c=_PTR, nq=40, nc=50, d=16, t=1.0, n=5, tau=_PTR, cut=_PTR, loss=_PTR, lse=_PTR, pos=_PTR,
                 dq=_PTR, dc=_PTR, counts=_PTR, ws=_PTR, ws_bytes=0)


def _select(lib, a):
  return lib.tfrs_inbatch_mined_select(a["q"], a["c"], a["nq"], a["nc"], a["d"], a["t"], None, None, None, a["n"],
                                       a["tau"], a["cut"], a["ws"], a["ws_bytes"], None)


def _fwd(lib, a):
  return lib.tfrs_inbatch_mined_ce_fwd(a["q"], a["c"], a["nq"], a["nc"], a["d"], None, a["t"], None, None, None,
                                       a["tau"], a["cut"], a["loss"], a["lse"], a["pos"], a["ws"], a["ws_bytes"], None)


def _bwd(lib, a):
  return lib.tfrs_inbatch_mined_ce_bwd(a["q"], a["c"], a["nq"], a["nc"], a["d"], None, a["t"], None, None, None,
                                       a["tau"], a["cut"], a["lse"], None, a["dq"], a["dc"], a["ws"], a["ws_bytes"],
                                       None)


def _count(lib, a):
  return lib.tfrs_inbatch_mined_rank_count(a["q"], a["c"], a["nq"], a["nc"], a["d"], a["t"], None, None, None,
                                           a["tau"], a["cut"], a["counts"], a["ws"], a["ws_bytes"], None)


_CALLS = {"inbatch_mined_select": _select, "inbatch_mined_ce_fwd": _fwd, "inbatch_mined_ce_bwd": _bwd,
          "inbatch_mined_rank_count": _count}


@pytest.mark.parametrize("over,names", [
    (dict(nq=0), "bad shape"),
    (dict(d=0), "bad shape"),
    (dict(d=129), "dim=129"),
    (dict(nq=51), "num_candidates >= num_queries"),
    (dict(q=None), "NULL"),
    (dict(c=None), "NULL"),
    (dict(ws=None), "NULL workspace"),
    (dict(t=0.0), "temperature"),
    (dict(t=float("nan")), "temperature"),
    (dict(), "workspace too small"),                 # every argument good, a workspace of 0 bytes
])
@pytest.mark.parametrize("who", sorted(_CALLS))
def test_entry_points_validate_before_they_touch_the_device(lib, who, over, names):
  """Every refusal is TFRS_EINVAL with the entry point named, on a host without a GPU: nothing has been launched.  The
  pointers are host addresses, so a call that got past its checks would not come back with TFRS_EINVAL."""
  from recommenders_amd import _lib
  assert _CALLS[who](lib, dict(_DEFAULTS, **over)) == _lib.TFRS_EINVAL
  assert who in _lib.last_error() and names in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("who,over,names", [
    ("inbatch_mined_select", dict(n=-1), "num_hard_negatives=-1"),
    ("inbatch_mined_select", dict(tau=None), "NULL output"),
    ("inbatch_mined_select", dict(cut=None), "NULL output"),
    ("inbatch_mined_ce_fwd", dict(loss=None), "NULL output"),
    ("inbatch_mined_ce_fwd", dict(tau=None), "tau and cut come together"),
    ("inbatch_mined_ce_bwd", dict(lse=None), "NULL pointer"),
    ("inbatch_mined_ce_bwd", dict(dc=None), "NULL pointer"),
    ("inbatch_mined_ce_bwd", dict(cut=None), "tau and cut come together"),
    ("inbatch_mined_rank_count", dict(counts=None), "NULL output"),
])
def test_entry_points_validate_their_own_arguments(lib, who, over, names):
  from recommenders_amd import _lib
  assert _CALLS[who](lib, dict(_DEFAULTS, **over)) == _lib.TFRS_EINVAL
  assert who in _lib.last_error() and names in _lib.last_error(), _lib.last_error()


def test_workspace_bytes_and_a_short_workspace(lib):
  from recommenders_amd import _lib
  ws = lib.tfrs_inbatch_mined_workspace_bytes
  base = int(ws(4096, 16384, 32))
  assert base >= 4096 * 256 * 4                                  # the selection's bins at least
  assert base <= 32 << 20                                        # ... and nothing like a logits matrix (256 MB)
  assert int(ws(4096, 16384, 64)) > base
  small = int(ws(40, 50, 16))
  for who, call in _CALLS.items():
    assert call(lib, dict(_DEFAULTS, ws_bytes=small - 1)) == _lib.TFRS_EINVAL
    assert who in _lib.last_error() and "workspace too small" in _lib.last_error()


# the shapes at which the GPU tests place ties across split boundaries, under the planner target they set
@pytest.mark.parametrize("nq,nc", [(33, 70), (64, 200), (40, 96)])
def test_plan_reports_three_or_more_splits_for_the_gpu_tests(lib, nq, nc):
  from recommenders_amd import _lib
  out = (ctypes.c_int64 * 4)()
  _lib.set_option("TFRS_SOFTMAX_WAVES", hb.GPU_TEST_WAVES)
  try:
    assert lib.tfrs_inbatch_mined_plan(nq, nc, out) == _lib.TFRS_OK
    many = list(out)
    _lib.set_option("TFRS_SOFTMAX_WAVES", "1")
    assert lib.tfrs_inbatch_mined_plan(nq, nc, out) == _lib.TFRS_OK
    one = list(out)
  finally:
    _lib.set_option("TFRS_SOFTMAX_WAVES", None)
  assert many[0] >= 3 and many[1] == 32                          # every candidate tile is a split of its own
  assert many[0] * many[1] >= nc and many[2] * many[3] >= nq
  assert one[0] == 1 and one[2] == 1
  f32 = (ctypes.c_int64 * 4)()
  _lib.set_option("TFRS_SOFTMAX_WAVES", hb.GPU_TEST_WAVES)
  try:
    assert lib.tfrs_inbatch_softmax_plan_f32(nq, 1, nc, f32) == _lib.TFRS_OK
  finally:
    _lib.set_option("TFRS_SOFTMAX_WAVES", None)
  assert list(f32) == many                                       # the planner of the f32 kernels
  assert lib.tfrs_inbatch_mined_plan(nc + 1, nc, out) == _lib.TFRS_EINVAL
  assert "inbatch_mined_plan" in _lib.last_error()


# ------------------------------------------------------------------------------------------ the compiled kernels
def test_mined_kernels_use_no_scratch_and_pass_the_mfma_hazard_checker():
  import importlib.util
  import subprocess
  import tempfile
  from recommenders_amd.csrc import build as csrc_build
  src = os.path.join(os.path.dirname(csrc_build.__file__), "softmax_mined.hip")
  out = os.path.join(tempfile.mkdtemp(prefix="tfrs_mined_"), "softmax_mined.s")
  subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17", "-S",
                  "--cuda-device-only", "-o", out, src], check=True, capture_output=True, cwd=os.path.dirname(src))
  with open(out) as f:
    asm = f.read()
  found = {"mined_scan_kernel": 0, "mined_bwd_kernel": 0}
  for block in asm.split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", block).group(1)
    for key in found:
      found[key] += key in name
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  assert found == {"mined_scan_kernel": 25, "mined_bwd_kernel": 10}       # 5 padded dims x 5 modes / x {dq, dc}
  # the temperature divides: the correctly rounded sequence, not a reciprocal multiply
  assert "v_div_fixup_f32" in asm and "v_div_fmas_f32" in asm
  spec = importlib.util.spec_from_file_location("check_mfma_hazards",
                                                os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  res = mod.check(asm)
  assert not {k: v[:3] for k, v in res.items() if v}
