"""Multi-head (max-sim) queries without a GPU: the float64 restatement the GPU tests compare against (the reference's
known answer, the single-head oracle, numerical derivatives, the tie rule), the new C entry points (header, library,
binding, argument checks before the device is touched) and the cross-compiled kernels (MFMA wait states, no
scratch)."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import retrieval as o_ret
from tests import multihead_restatement as mh
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tfrs_inbatch_softmax_mh_workspace_bytes", "tfrs_inbatch_softmax_mh_ce_fwd",
               "tfrs_inbatch_softmax_mh_ce_bwd", "tfrs_topk_merge_heads")


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_reference_max_sim_known_answer():
  case = [c for c in load_golden("retrieval.json")["cases"] if np.asarray(c["query"]).ndim == 3]
  assert len(case) == 1                                                  # tasks/retrieval_test.py:257-298
  case = case[0]
  got = mh.loss(np.asarray(case["query"], np.float32), np.asarray(case["candidate"], np.float32))
  assert got == pytest.approx(case["expected_loss"], rel=1e-6)
  assert got == pytest.approx(float(o_ret.loss(np.asarray(case["query"], np.float32),
                                               np.asarray(case["candidate"], np.float32))), rel=1e-6)


def _options(rng, nq, nc):
  w = rng.uniform(0.1, 2.0, size=nq).astype(np.float32)
  p = rng.uniform(0.0, 1.0, size=nc).astype(np.float32)
  p[::7] = 0.0                                                           # the 1e-6 clip
  ids = rng.integers(0, max(nc // 3, 2), size=nc)                        # duplicates: accidental hits
  mask = rng.uniform(size=(nq, nc)) > 0.2
  mask[np.arange(nq), np.arange(nq)] = True
  return [dict(), dict(sample_weight=w), dict(temperature=0.7), dict(candidate_sampling_probability=p),
          dict(candidate_ids=ids), dict(score_mask=mask),
          dict(sample_weight=w, temperature=1.3, candidate_sampling_probability=p, candidate_ids=ids,
               score_mask=mask)]


def test_with_one_head_the_restatement_is_the_single_head_oracle():
  rng = np.random.default_rng(5)
  nq, nc, d = 23, 37, 12
  q = rng.normal(size=(nq, d)).astype(np.float32)
  c = rng.normal(size=(nc, d)).astype(np.float32)
  for kw in _options(rng, nq, nc):
    okw = dict(kw)
    if "candidate_ids" in okw:
      okw["remove_accidental_hits_flag"] = True
    assert mh.loss(q[:, None, :], c, **kw) == pytest.approx(float(o_ret.loss(q, c, **okw)), rel=2e-6)
    dq, dc, dq_y, dc_y = mh.loss_grads(q[:, None, :], c, return_yardsticks=True, **kw)
    rq, rc, rq_y, rc_y = o_ret.loss_grads(q, c, return_yardsticks=True, **okw)
    # the oracle forms its logits in float32: a few 2^-24 of the yardstick
    assert np.all(np.abs(dq[:, 0] - rq) <= 2e-6 * rq_y + 1e-30)
    assert np.all(np.abs(dc - rc) <= 2e-6 * rc_y + 1e-30)
    np.testing.assert_allclose(dq_y[:, 0], rq_y, rtol=1e-5)
    np.testing.assert_allclose(dc_y, rc_y, rtol=1e-5)


def test_restatement_gradients_agree_with_central_differences():
  """float64 inputs without ties: the winner of every pair is constant in a neighbourhood, so the loss is smooth
  there and the analytic gradients are its derivatives."""
  rng = np.random.default_rng(11)
  nq, heads, nc, d = 5, 3, 7, 4
  q = rng.normal(size=(nq, heads, d))
  c = rng.normal(size=(nc, d))
  gap, _ = mh.head_gap_guard(q, c)
  assert gap > 1e-3
  for kw in _options(rng, nq, nc):
    dq, dc = mh.loss_grads(q, c, **kw)
    eps = 1e-6
    for arr, grad in ((q, dq), (c, dc)):
      num = np.zeros_like(arr)
      it = np.nditer(arr, flags=["multi_index"])
      for _ in it:
        i = it.multi_index
        keep = arr[i]
        arr[i] = keep + eps
        up = mh.loss(q, c, **kw)
        arr[i] = keep - eps
        down = mh.loss(q, c, **kw)
        arr[i] = keep
        num[i] = (up - down) / (2 * eps)
      np.testing.assert_allclose(grad, num, rtol=1e-5, atol=1e-7)


def test_restatement_gives_a_duplicated_head_no_gradient():
  rng = np.random.default_rng(13)
  q = rng.normal(size=(9, 3, 6)).astype(np.float32)
  c = rng.normal(size=(12, 6)).astype(np.float32)
  q[:, 1] = q[:, 0]
  dq, dc = mh.loss_grads(q, c, temperature=0.5)
  assert np.all(dq[:, 1] == 0.0) and np.abs(dq[:, 0]).sum() > 0
  # ... and the pair of copies gets what the single head gets without the copy
  dq1, dc1 = mh.loss_grads(q[:, [0, 2]], c, temperature=0.5)
  np.testing.assert_array_equal(dq[:, [0, 2]], dq1)
  np.testing.assert_array_equal(dc, dc1)


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
  with open(os.path.join(ROOT, "include", "tfrs_hip.h")) as f:
    header = f.read()
  for name in NEW_SYMBOLS:
    assert re.search(r"\b%s\(" % name, header), name
    assert hasattr(lib, name), name
    assert name in _lib.SIGNATURES, name
  assert "softmax.hip" in csrc_build.SOURCES                     # the multi-head kernels live in the merged file
  assert not os.path.exists(os.path.join(os.path.dirname(csrc_build.__file__), "softmax_mh.hip"))


_BUF = ctypes.create_string_buffer(64)            # a non-NULL host address: never dereferenced by a refused call
_PTR = ctypes.c_void_p(ctypes.addressof(_BUF))

_SOFTMAX_DEFAULTS = dict(q=_PTR, c=_PTR, nq=40, heads=3, nc=50, d=16, loss=_PTR, lse=_PTR, pos=_PTR, dq=_PTR, dc=_PTR,
                         ws=_PTR, ws_bytes=0)


def _fwd(lib, **over):
  a = dict(_SOFTMAX_DEFAULTS, **over)
  return lib.tfrs_inbatch_softmax_mh_ce_fwd(a["q"], a["c"], a["nq"], a["heads"], a["nc"], a["d"], None, 1.0, None,
                                            None, None, a["loss"], a["lse"], a["pos"], a["ws"], a["ws_bytes"], None)


def _bwd(lib, **over):
  a = dict(_SOFTMAX_DEFAULTS, **over)
  return lib.tfrs_inbatch_softmax_mh_ce_bwd(a["q"], a["c"], a["nq"], a["heads"], a["nc"], a["d"], None, 1.0, None,
                                            None, None, a["lse"], None, a["dq"], a["dc"], a["ws"], a["ws_bytes"],
                                            None)


@pytest.mark.parametrize("over,names", [
    (dict(heads=0), "heads=0"),
    (dict(heads=33), "heads=33"),
    (dict(d=129), "dim=129"),
    (dict(d=0), "dim=0"),
    (dict(nq=51), "num_candidates >= num_queries"),
    (dict(q=None), "NULL"),
    (dict(c=None), "NULL"),
    (dict(lse=None), "NULL"),
    (dict(ws=None), "NULL"),
    (dict(), "workspace too small"),                 # every argument good, a workspace of 0 bytes
])
@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_softmax_entry_points_validate_before_they_touch_the_device(lib, call, over, names):
  """Every refusal is TFRS_EINVAL with the argument named, on a host without a GPU: nothing has been launched.  The
  pointers are host addresses, so a call that got past its checks would not come back with TFRS_EINVAL."""
  from recommenders_amd import _lib
  assert call(lib, **over) == _lib.TFRS_EINVAL
  name = "inbatch_softmax_mh_ce_fwd" if call is _fwd else "inbatch_softmax_mh_ce_bwd"
  assert name in _lib.last_error() and names in _lib.last_error(), _lib.last_error()


def test_softmax_workspace_bytes(lib):
  ws = lib.tfrs_inbatch_softmax_mh_workspace_bytes
  base = int(ws(64, 4, 128, 32))
  assert base >= (64 * 4 + 128) * 32 * 4                       # one partial gradient of each side at least
  assert int(ws(64, 8, 128, 32)) > base and int(ws(64, 4, 128, 64)) > base and int(ws(64, 4, 256, 32)) > base
  short = base - 1
  from recommenders_amd import _lib
  assert _fwd(lib, nq=64, heads=4, nc=128, d=32, ws_bytes=short) == _lib.TFRS_EINVAL
  assert "workspace too small" in _lib.last_error()


def _merge(lib, **over):
  a = dict(dict(scores=None, rows=None, nq=0, heads=4, k_in=10, k_out=10, out_s=None, out_r=None), **over)
  return lib.tfrs_topk_merge_heads(a["scores"], a["rows"], a["nq"], a["heads"], a["k_in"], a["k_out"], a["out_s"],
                                   a["out_r"], None)


@pytest.mark.parametrize("over,names", [
    (dict(heads=0), "heads=0"),
    (dict(heads=33), "heads=33"),
    (dict(heads=4, k_in=1025, k_out=10), "k_in=1025"),
    (dict(heads=3, k_in=2731, k_out=1), "heads * k_in = 8193"),
    (dict(heads=1, k_in=8193, k_out=1), "heads * k_in = 8193"),
    (dict(heads=8, k_in=1025, k_out=10), "heads * k_in = 8200"),
    (dict(heads=32, k_in=257, k_out=257), "heads * k_in = 8224"),
    (dict(k_in=0), "k_in=0"),
    (dict(k_out=11), "k_out=11"),
    (dict(k_out=0), "k_out=0"),
    (dict(nq=-1), "nq=-1"),
    (dict(nq=3), "NULL"),
    (dict(nq=3, scores=_PTR, rows=_PTR, out_s=_PTR), "NULL"),
])
def test_merge_heads_validates_before_it_touches_the_device(lib, over, names):
  from recommenders_amd import _lib
  assert _merge(lib) == _lib.TFRS_OK                                       # nq = 0 with good arguments: nothing to do
  assert _merge(lib, heads=8, k_in=1024, k_out=1024) == _lib.TFRS_OK      # the 8192-pair edge is inside
  assert _merge(lib, **over) == _lib.TFRS_EINVAL
  assert "topk_merge_heads" in _lib.last_error() and names in _lib.last_error(), _lib.last_error()


# ------------------------------------------------------------------------------------------ the compiled kernels
_ASM = {}


def _asm(src_name):
  if src_name not in _ASM:
    from recommenders_amd.csrc import build as csrc_build
    src = os.path.join(os.path.dirname(csrc_build.__file__), src_name)
    out = os.path.join(tempfile.mkdtemp(prefix="tfrs_mh_"), src_name + ".s")
    subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17",
                    *csrc_build.EXTRA_FLAGS.get(src_name, []), "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True, cwd=os.path.dirname(src))
    with open(out) as f:
      _ASM[src_name] = f.read()
  return _ASM[src_name]


# the kernels of softmax.hip by their last template argument, MH (mangled: Lb1E = true, Lb0E = false)
_SOFTMAX_KERNEL = r"softmax_%s_kernelI\w*Lb%dEEEv"


def test_multi_head_softmax_kernels_pass_the_mfma_hazard_checker():
  import importlib.util
  spec = importlib.util.spec_from_file_location("check_mfma_hazards",
                                                os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  res = mod.check(_asm("softmax.hip"))
  for mh in (1, 0):
    assert sum(bool(re.search(_SOFTMAX_KERNEL % ("fwd", mh), name)) for name in res) == 10   # 5 padded dims x {plain, options}
    assert sum(bool(re.search(_SOFTMAX_KERNEL % ("bwd", mh), name)) for name in res) == 20   # ... x {dq, dc}
  assert not {k: v[:3] for k, v in res.items() if v}


@pytest.mark.parametrize("src_name,pattern,count", [
    pytest.param("softmax.hip", _SOFTMAX_KERNEL % ("(fwd|bwd)", 1), 30, id="softmax.hip-multi_head-30"),
    pytest.param("softmax.hip", _SOFTMAX_KERNEL % ("(fwd|bwd)", 0), 30, id="softmax.hip-single_head-30"),
    ("topk_merge_heads.hip", "merge_heads", 1)])
def test_new_kernels_use_no_scratch(src_name, pattern, count):
  found = 0
  for block in _asm(src_name).split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", block).group(1)
    if not re.search(pattern, name):
      continue
    found += 1
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  assert found == count
