"""factorized_top_k.ScaNN without a GPU: import, constructor validation, the host probe planner (property-tested), the
argument checks of tfrs_scann_search and its workspace size, and the cross-compiled scan kernels (MFMA wait states, no
scratch)."""

import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st


def _ftk():
  from recommenders_amd.layers import factorized_top_k
  return factorized_top_k


def test_scann_is_importable():
  from recommenders_amd.layers.factorized_top_k import ScaNN, TopK
  assert issubclass(ScaNN, TopK)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(distance_measure="squared_l2"), NotImplementedError),
    (dict(distance_measure="cosine"), NotImplementedError),
    (dict(k=1025), ValueError),
    (dict(k=0), ValueError),
    (dict(num_reordering_candidates=1025), ValueError),
    (dict(num_reordering_candidates=0), ValueError),
    (dict(num_leaves=0), ValueError),
    (dict(num_leaves_to_search=0), ValueError),
    (dict(dimensions_per_block=0), ValueError),
    (dict(training_iterations=-1), ValueError),
])
def test_constructor_validation(kwargs, exc):
  with pytest.raises(exc):
    _ftk().ScaNN(**kwargs)


def test_constructor_accepts_reference_arguments():
  layer = _ftk().ScaNN(None, 10, "dot_product", 100, 10, 12, 2, None, True, "scann", seed=3)
  assert layer.name == "scann" and not layer.is_exact()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_without_gpu_the_layer_fails_loudly():
  layer = _ftk().ScaNN()
  with pytest.raises(RuntimeError, match="GPU"):
    layer.index(np.zeros((100, 4), dtype=np.float32))


def test_call_before_index_raises():
  with pytest.raises(ValueError, match="index"):
    _ftk().ScaNN()(np.zeros((2, 4), dtype=np.float32))


@settings(max_examples=300, deadline=None)
@given(sizes=st.lists(st.integers(0, 50), min_size=1, max_size=40), nls=st.integers(1, 45), k=st.integers(1, 200))
def test_probe_plan_properties(sizes, nls, k):
  """Every choice of L_eff leaves holds >= k rows; when L_eff was widened, some choice of L_eff - 1 leaves holds fewer;
  P_max is the largest possible probe."""
  plan = _ftk().scann_probe_plan
  sizes = np.asarray(sizes)
  if sizes.sum() < k:
    with pytest.raises(ValueError):
      plan(sizes, nls, k)
    return
  l_eff, p_max = plan(sizes, nls, k)
  asc, desc = np.sort(sizes), np.sort(sizes)[::-1]
  assert min(nls, len(sizes)) <= l_eff <= len(sizes)
  assert asc[:l_eff].sum() >= k                                   # the worst choice of L_eff leaves
  if l_eff > min(nls, len(sizes)):
    assert asc[:l_eff - 1].sum() < k
  assert p_max == desc[:l_eff].sum()


def test_probe_plan_examples():
  plan = _ftk().scann_probe_plan
  assert plan([10] * 100, 10, 10) == (10, 100)
  assert plan([5, 1, 1, 100], 2, 3) == (3, 106)
  assert plan([5, 1, 1, 100], 9, 3) == (4, 107)


@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


_SEARCH_DEFAULTS = dict(nq=0, d=20, l_eff=3, num_leaves=8, max_leaf_rows=100, code_bytes=8, dims_per_block=2,
                        lut_exp=0, p_max=300, r=20, k=10)


def _search(lib, **over):
  """tfrs_scann_search with NULL pointers and one or more arguments changed: validation only, nothing is launched."""
  a = dict(_SEARCH_DEFAULTS, **over)
  return lib.tfrs_scann_search(None, a["nq"], a["d"], None, None, a["l_eff"], None, a["num_leaves"],
                               a["max_leaf_rows"], None, a["code_bytes"], None, a["dims_per_block"], a["lut_exp"],
                               None, None, a["p_max"], a["r"], a["k"], None, None, None, 0, None)


@pytest.mark.parametrize("over,names", [
    (dict(code_bytes=6), "code_bytes=6"),                                    # not a multiple of 4
    (dict(code_bytes=68), "code_bytes=68"),                                  # above the 64-byte ceiling
    (dict(d=128, dims_per_block=1, code_bytes=60), "code_bytes=60"),         # 128 blocks need 64 bytes
    (dict(r=5), "r=5"),                                                      # r < k
    (dict(r=1025), "r=1025"),
    (dict(p_max=5), "p_max=5"),                                              # p_max < k
    (dict(l_eff=9), "l_eff=9"),                                              # above num_leaves = 8
    (dict(dims_per_block=21), "dims_per_block=21"),                          # above d = 20
    (dict(d=129, dims_per_block=2), "dim=129"),
    (dict(nq=1 << 20, l_eff=4096, num_leaves=4096), "nq * l_eff"),           # 2^32 (query, probe) pairs
])
def test_search_validates_before_it_touches_the_device(lib, over, names):
  """Every argument check of tfrs_scann_search comes before its nq == 0 return and before any HIP call: with nq = 0
  (or NULL pointers) a bad argument is TFRS_EINVAL and tfrs_last_error names it; the same call with good arguments
  is TFRS_OK."""
  from recommenders_amd import _lib
  assert _search(lib) == _lib.TFRS_OK
  assert _search(lib, **over) == _lib.TFRS_EINVAL
  assert "scann_search" in _lib.last_error() and names in _lib.last_error(), _lib.last_error()


def test_search_workspace_bytes(lib):
  """0 for a non-positive argument, growing with every argument, and capped in r at p_max (the selection never holds
  more than the score row)."""
  ws = lib.tfrs_scann_search_workspace_bytes
  base = dict(nq=64, num_leaves=100, l_eff=10, d=20, p_max=5000, r=100)
  order = ("nq", "num_leaves", "l_eff", "d", "p_max", "r")
  size = lambda **over: int(ws(*[dict(base, **over)[name] for name in order]))
  assert size() > 4 * 64 * 5000
  for name in order:
    assert size(**{name: 0}) == 0, name
    assert size(**{name: -1}) == 0, name
    assert size(**{name: 2 * base[name]}) > size(), name
  assert size(r=5000) == size(r=5001) == size(r=1 << 20)


_ASM = {}


def _scann_asm():
  if "s" not in _ASM:
    from recommenders_amd.csrc import build as csrc_build
    src = os.path.join(os.path.dirname(csrc_build.__file__), "scann.hip")
    out = os.path.join(tempfile.mkdtemp(prefix="tfrs_scann_"), "scann.s")
    subprocess.run([csrc_build.hipcc(), f"--offload-arch={csrc_build.ARCH}", "-O3", "-std=c++17",
                    *csrc_build.EXTRA_FLAGS.get("scann.hip", []), "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True, cwd=os.path.dirname(src))
    with open(out) as f:
      _ASM["s"] = f.read()
  return _ASM["s"]


def test_scann_source_is_built():
  from recommenders_amd.csrc import build as csrc_build
  assert "scann.hip" in csrc_build.SOURCES


def test_scann_kernels_pass_the_mfma_hazard_checker():
  import importlib.util
  path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_mfma_hazards.py")
  spec = importlib.util.spec_from_file_location("check_mfma_hazards", path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  res = mod.check(_scann_asm())
  assert sum("scann_scan_kernel" in name for name in res) == 8
  assert not {k: v[:3] for k, v in res.items() if v}


def test_scann_kernels_use_no_scratch():
  found = 0
  for block in _scann_asm().split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", block).group(1)
    if "scann" not in name:
      continue
    found += 1
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
  assert found == 15     # zero, slots, plan, scatter, qprep, fill, map and the scan for 1..8 k-steps
