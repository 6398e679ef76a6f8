"""The 16x16x32 arm of the fp16 scan kernels (csrc/topk_scan16.hip, template parameter MF / TFRS_SCAN16_MFMA) on the
cross-compiled gfx950 assembly: which instantiations exist, which MFMA they issue, their register budget, and the
hazard checker's arithmetic for the 4-pass shape.  No GPU needed."""
import re

import pytest

from tests.test_host_cpu import _device_asm, _mfma_hazard_checker

# <DP, waves, groups, stages per period, NT, MF> / <DP, mode, NT, MF>; mode 1 = MATERIALIZE, 2 = BINMAX
FILTER_16 = "scan16f_kernelILi64ELi16ELi2ELi2ELb0ELi16EE"
FILTER_32 = "scan16f_kernelILi64ELi16ELi2ELi2ELb0ELi32EE"
BINMAX_16 = "scan16_kernelILi64ELi2ELb0ELi16EE"
BINMAX_32 = "scan16_kernelILi64ELi2ELb0ELi32EE"


def _kernels():
  """{mangled name: (body, metadata block)} of topk_scan16.hip."""
  asm = _device_asm("topk_scan16.hip")
  bodies = dict(_mfma_hazard_checker().kernels(asm))
  meta = {}
  for block in asm.split("- .agpr_count:")[1:]:
    meta[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
  assert set(meta) <= set(bodies)
  return {k: ("\n".join(t for _, t in bodies[k]), meta[k]) for k in meta}


def _one(kernels, pattern):
  hit = [k for k in kernels if pattern in k]
  assert len(hit) == 1, (pattern, hit)
  return kernels[hit[0]]


def test_each_arm_issues_its_own_mfma_shape():
  """The default dim-64 filter instantiation and the threshold pass exist in both shapes, and each issues ONE shape."""
  ks = _kernels()
  for pattern in (FILTER_16, BINMAX_16):
    body, _ = _one(ks, pattern)
    assert "v_mfma_f32_16x16x32_f16" in body and "32x32x16" not in body, pattern
  for pattern in (FILTER_32, BINMAX_32):
    body, _ = _one(ks, pattern)
    assert "v_mfma_f32_32x32x16_f16" in body and "16x16x32" not in body, pattern
  # 8 instructions of 16 cycles per 32 x 32 x 64 tile instead of 4 of 32: two stages x 4 sub-tiles x 2 groups
  assert _one(ks, FILTER_16)[0].count("v_mfma_f32_16x16x32_f16") == 2 * _one(ks, FILTER_32)[0].count("v_mfma_f32_32x32x16_f16")


def test_which_instantiations_have_the_16x16_arm():
  """Both shapes for what the launchers pick by default at dims 32, 64, 128 -- <DP, 16, 2, 2> (up to 64), <DP, 8, 2>
  with and without the non-temporal copies, BINMAX with and without, MATERIALIZE; dim 16 (K = 32 per instruction does
  not fit), the first-generation FILTER and the A/B-only workgroup shapes stay 32x32."""
  names = set(_kernels())
  has = lambda sub: any(sub in n for n in names)
  for dp in (32, 64, 128):
    for mf in (16, 32):
      assert has(f"scan16f_kernelILi{dp}ELi8ELi2ELi1ELb0ELi{mf}EE") and has(f"scan16f_kernelILi{dp}ELi8ELi2ELi1ELb1ELi{mf}EE")
      assert has(f"scan16_kernelILi{dp}ELi2ELb0ELi{mf}EE") and has(f"scan16_kernelILi{dp}ELi2ELb1ELi{mf}EE")
      assert has(f"scan16_kernelILi{dp}ELi1ELb0ELi{mf}EE")
      if dp <= 64:
        assert has(f"scan16f_kernelILi{dp}ELi16ELi2ELi2ELb0ELi{mf}EE")
  sixteen = {n for n in names if n.endswith("ELi16EEEvNS_10Scan16ArgsE")}
  assert sixteen and not [n for n in sixteen if "kernelILi16E" in n]                       # no dim 16
  assert not [n for n in sixteen if re.search(r"scan16_kernelILi\d+ELi0E", n)]              # no first-generation FILTER
  assert not [n for n in sixteen if re.search(r"scan16f_kernelILi\d+E(Li4ELi4|Li8ELi4|Li16ELi2ELi1)E", n)]


def test_the_diagnostic_peel_build_has_no_16x16_arm():
  """TFRS_SCAN16_PEEL=1 is the hazard checker's known positive (tests/test_host_cpu.py): it keeps the 32x32 kernels
  only, so every kernel of that build whose name starts like the default filter instantiation shows the fault."""
  asm = _device_asm("topk_scan16.hip", ("TFRS_SCAN16_PEEL=1",))
  assert "v_mfma_f32_32x32x16_f16" in asm and "v_mfma_f32_16x16x32_f16" not in asm


@pytest.mark.parametrize("pattern,max_vgprs", [
    (FILTER_16, 128), ("scan16f_kernelILi64ELi8ELi2ELi1ELb0ELi16EE", 128), ("scan16f_kernelILi64ELi8ELi2ELi1ELb1ELi16EE", 128),
    ("scan16f_kernelILi32ELi16ELi2ELi2ELb0ELi16EE", 128), ("scan16f_kernelILi32ELi8ELi2ELi1ELb0ELi16EE", 128),
    (BINMAX_16, 128), ("scan16_kernelILi64ELi2ELb1ELi16EE", 128), ("scan16_kernelILi64ELi1ELb0ELi16EE", 128),
    # dim 128: two waves per SIMD
    ("scan16f_kernelILi128ELi8ELi2ELi1ELb0ELi16EE", 256), ("scan16_kernelILi128ELi2ELb0ELi16EE", 256),
])
def test_16x16_kernels_keep_the_register_budget(pattern, max_vgprs):
  """Four waves per SIMD up to dim 64 (<= 128 VGPRs), no spills, no scratch: named one by one, not by a shared prefix."""
  _, meta = _one(_kernels(), pattern)
  assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
  assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
  assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
  assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= max_vgprs


def test_16x16_kernels_wait_for_the_matrix_pipe():
  """The max tree reads its accumulators 8 wait states behind the chain's last v_mfma_f32_16x16x32_f16 at the
  earliest -- hand-written in the filter kernel (`s_nop 7`), the compiler's in the threshold pass -- on every path
  the checker walks."""
  res = _mfma_hazard_checker().check(_device_asm("topk_scan16.hip"))
  mine = {k: v for k, v in res.items() if k.endswith("ELi16EEEvNS_10Scan16ArgsE")}
  assert len(mine) >= 17
  assert not {k: v[:3] for k, v in mine.items() if v}


def test_the_query_prologue_of_the_16x16_kernels_keeps_its_loads_in_flight():
  """Same property as tests/test_host_cpu.py::test_pipelined_kernels_keep_loads_in_flight, for the new names: the
  16 x 16-byte query loads of a wave are issued before the first wait."""
  ks = _kernels()
  for pattern in (FILTER_16, BINMAX_16):
    waits = [int(v) for v in re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", _one(ks, pattern)[0])]
    assert waits and max(waits) >= 8, (pattern, sorted(set(waits))[-5:])


def test_hazard_checker_counts_8_wait_states_behind_the_4_pass_shape():
  chk = _mfma_hazard_checker()

  def listing(body):
    return "_Z1kv:\n" + "\n".join("\t" + l for l in body) + "\n\t.amdhsa_kernel _Z1kv\n"

  mf = "v_mfma_f32_16x16x32_f16 v[0:3], v[20:23], v[24:27], v[0:3]"
  assert chk.check(listing([mf, "s_nop 7", "v_max3_f32 v40, v0, v1, v2"])) == {"_Z1kv": []}              # 8
  assert chk.check(listing([mf, "s_nop 4", "v_mov_b32_e32 v50, v51", "s_nop 1", "v_max3_f32 v40, v0, v1, v2"])) == {"_Z1kv": []}
  (bad,) = chk.check(listing([mf, "s_nop 6", "v_max3_f32 v40, v0, v1, v2"]))["_Z1kv"]                   # 7
  assert bad[1].startswith("v_max3_f32") and bad[3] == 1
  # four accumulators of a tile: the wait is counted per accumulator, from ITS last link
  other = "v_mfma_f32_16x16x32_f16 v[4:7], v[20:23], v[28:31], v[4:7]"
  assert chk.check(listing([mf, other, "s_nop 6", "v_max3_f32 v40, v0, v1, v2"])) == {"_Z1kv": []}       # 1 + 7 behind v[0:3]
  (bad,) = chk.check(listing([mf, other, "s_nop 6", "ds_write_b128 v50, v[4:7]"]))["_Z1kv"]              # 7 behind v[4:7]
  assert bad[1].startswith("ds_write_b128") and bad[3] == 1
