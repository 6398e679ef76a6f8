"""The hand-built operands of tests/gemm_handbuilt.py, proved on the host: the exactness conditions of both families are
derived again from the arrays alone, in int64 / float64 and with numpy float16 restating the hi / lo split, and the
launch geometry every case of tests/test_gemm_layout_gpu.py claims is asked from the library's own planner
(``tfrs_gemm_plan``: the functions the launchers call).  No GPU access: the plan entry point does no device work."""

import contextlib
import ctypes

import numpy as np
import pytest

from recommenders_amd import _lib
from tests import gemm_handbuilt as hb


def lib_plan(f16, m, n, k, flags=0, align=0):
  out = (ctypes.c_int64 * 20)()
  _lib.check(_lib.load().tfrs_gemm_plan(f16, m, n, k, flags, align, out))
  return list(out)


@contextlib.contextmanager
def options(tile=0, splitk=None):
  try:
    _lib.set_option("TFRS_GEMM16_TILE", str(tile) if tile else None)
    _lib.set_option("TFRS_GEMM16_SPLITK", None if splitk is None else str(splitk))
    yield
  finally:
    _lib.set_option("TFRS_GEMM16_TILE", None)
    _lib.set_option("TFRS_GEMM16_SPLITK", None)


# ------------------------------------------------------------------------------------------ the plan entry
def test_plan_entry_point_rejects_bad_arguments():
  lib, out = _lib.load(), (ctypes.c_int64 * 20)()
  bad = [(1, 0, 5, 5, 0, 0), (1, 5, 0, 5, 0, 0), (1, 5, 5, 0, 0, 0), (0, -1, 5, 5, 0, 0), (2, 5, 5, 5, 0, 0),
         (-1, 5, 5, 5, 0, 0), (1, 5, 5, 5, 128, 0), (1, 5, 5, 5, -1, 0), (1, 5, 5, 5, 0, 1), (1, 5, 5, 5, 0, 0x20),
         (1, 5, 5, 5, 0, 0x10000), (1, 5, 5, 5, 0, -4), (0, 5, 5, 5, hb.AT | hb.BT, 0), (1, 5, 5, 1 << 31, 0, 0),
         (1, 1 << 31, 5, 5, 0, 0)]
  for args in bad:
    assert lib.tfrs_gemm_plan(*args, out) == _lib.TFRS_EINVAL, args
  assert lib.tfrs_gemm_plan(1, 5, 5, 5, 0, 0, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_gemm_plan(1, 5, 5, 5, hb.AT | hb.BT, 0xCCCC, out) == _lib.TFRS_OK      # (f16 has A^T B^T)
  assert lib_plan(0, 129, 131, 2049, hb.AT)[:7] == [2, 1040, 2, 1009, 0, 0, 4]


FLAG_SWEEP = (0, hb.BT, hb.AT, hb.AT | hb.BMUL, hb.BT | hb.AMUL | hb.EPI, hb.BIAS, hb.ACT | hb.EPI, hb.AT | hb.BT)
ALIGN_SWEEP = (0, 0x4, 0x8, 0x40, 0x80, 0xC0, 0x400, 0x800, 0x8000, 0x4000)


def test_restated_planner_equals_the_librarys_over_a_sweep():
  ms = (1, 127, 129, 257, 300, 4097, 65536)
  ns = (1, 3, 131, 256, 257, 3456, 8196)
  ks = (1, 13, 63, 64, 65, 300, 1030, 2047, 2048, 2049, 2050, 3073, 4096, 4100, 5082, 8191, 8192, 8194, 8196, 12287,
        12288, 12289, 16385, 20000, 65536, 131072)
  seen = set()
  for tile, splitk in ((0, None), (128, None), (256, None), (0, 3), (256, 40)):
    with options(tile, splitk):
      for m in ms:
        for n in ns:
          for k in ks:
            for flags in FLAG_SWEEP:
              for align in ALIGN_SWEEP if k in (300, 1030, 2048, 8192) or m == 129 else (0,):
                got = lib_plan(1, m, n, k, flags, align)
                assert got == hb.plan(1, m, n, k, flags, align, tile, splitk), (1, m, n, k, flags, align, tile, splitk)
                seen.add((got[0], got[10], got[11], got[12], got[13]))
                if tile == 0 and splitk is None and not (flags & hb.AT and flags & hb.BT):
                  assert lib_plan(0, m, n, k, flags, align) == hb.plan(0, m, n, k, flags, align), (0, m, n, k, flags, align)
  # the 16 Mi-float cap of the f32 split: no more than 16 Mi / (m n) slices
  # (1500 x 1500 = 144 tiles ask for 8 slices and get 16 Mi / 2.25 M = 7; 256 tiles and more do not split)
  assert lib_plan(0, 1500, 1500, 65536, hb.AT)[:3] == [7, 9376, 7] and hb.splitk_slices_f32(1500, 1500, 65536) == 7
  assert lib_plan(0, 1024, 1024, 65536, hb.AT)[:3] == [16, 4096, 16] and lib_plan(0, 2048, 2048, 65536, hb.AT)[0] == 1
  # every row-prep variant the launcher has was asked for
  assert {s[1:] for s in seen if s[1] == hb.KIND_KSM1} == {(2, 2, 0, 4), (2, 4, 0, 4), (2, 8, 0, 4), (2, 16, 0, 4),
                                                           (2, 4, 1, 4), (2, 8, 1, 8)}


def test_every_product_of_the_gpu_file_has_the_plan_restated():
  for f16, m, n, k, flags, align, tile in hb.products():
    with options(tile):
      assert lib_plan(f16, m, n, k, flags, align) == hb.plan(f16, m, n, k, flags, align, tile), (f16, m, n, k, flags, align, tile)


def test_the_starting_table():
  """The shapes were chosen for what the planner does with them: said here in numbers."""
  d = lambda *a, **kw: hb.describe(1, *a, **kw)
  p = d(129, 131, 12289, hb.BT)
  assert (p["slices"], p["kt_per"], p["last"], p["count"] % 4, p["big"]) == (6, 129, 127, 3, 1)
  p = d(257, 129, 8192, hb.BT)
  assert (p["slices"], p["kt_per"], p["last"], p["mp"]) == (3, 171, 170, 512)
  p = d(130, 3, 20000, hb.BT)
  assert (p["slices"], p["last"], p["count"] % 4) == (6, 207, 2)
  p = d(300, 257, 16385, hb.BT)
  assert (p["slices"], p["kt_per"], p["last"], p["mp"], p["np"], p["count"] % 4) == (8, 129, 125, 512, 512, 0)
  assert d(129, 131, 8191, hb.BT)["slices"] == 1 and d(129, 131, 8192, hb.BT)["slices"] == 1
  assert d(129, 131, 12289, hb.BT | hb.EPI)["slices"] == 1 and d(129, 131, 12289, hb.BIAS)["big"] == 0
  want = {64: (2, 0, 4), 300: (2, 0, 4), 2048: (4, 0, 4), 4096: (8, 0, 4), 4100: (16, 0, 4), 8192: (16, 0, 4),
          1030: (4, 1, 4), 2050: (8, 1, 8), 5082: (8, 1, 8), 8196: (0, 0, 4), 8194: (0, 0, 4), 13: (0, 0, 4), 1: (0, 0, 4)}
  for k, (m, n) in hb.ROWPREP_K.items():
    for flags in (hb.BT, hb.BT | hb.AMUL | hb.EPI):
      a = d(m, n, k, flags, tile=256)["a"]
      assert (a["steps"], a["v2"], a["waves"]) == want[k] and a["kind"] == (hb.KIND_KSM1 if want[k][0] else hb.KIND_KSM2)
  for k, off, what in hb.ROWPREP_OFFSETS:
    a, b = d(129, 131, k, hb.BT, off, tile=256)["a"], d(129, 131, k, hb.BT, off << 4, tile=256)["b"]
    assert a == b and {"fallback": a["kind"] == hb.KIND_KSM2, "v2": a["kind"] == hb.KIND_KSM1 and a["v2"] == 1}[what]
    assert d(129, 131, k, hb.BT, 0, tile=256)["a"]["kind"] == hb.KIND_KSM1          # (the offset is what changes the path)
  f = lambda *a: hb.describe(0, *a, hb.AT)
  assert f(129, 131, 2047)["slices"] == 1 and (f(129, 131, 2048)["kper"], f(129, 131, 2048)["last"]) == (1024, 1024)
  assert (f(129, 131, 2049)["kper"], f(129, 131, 2049)["last"]) == (1040, 1009)
  assert (f(129, 131, 3073)["used"], f(129, 131, 3073)["last"]) == (3, 993)
  assert f(5, 3, 2100)["used"] == 2 and f(13, 512, 4097)["used"] == 4


def test_the_cases_reach_every_variant():
  """The geometry table: what the products of tests/test_gemm_layout_gpu.py reach, asked from the plans."""
  plans16 = [(fl, hb.describe(1, m, n, k, fl, al, tile)) for f16, m, n, k, fl, al, tile in hb.products() if f16]
  plans32 = [(fl, hb.describe(0, m, n, k, fl, al)) for f16, m, n, k, fl, al, tile in hb.products() if not f16]
  variants = {(2, 0, 4), (4, 0, 4), (8, 0, 4), (16, 0, 4), (4, 1, 4), (8, 1, 8), (0, 0, 4)}
  for mul in (0, hb.AMUL):                                   # every row-prep variant in both MUL states (A side) ...
    got = {(p["a"]["steps"], p["a"]["v2"], p["a"]["waves"]) for fl, p in plans16
           if p["a"]["kind"] in (hb.KIND_KSM1, hb.KIND_KSM2) and fl & hb.AMUL == mul}
    assert got == variants, (mul, got)
  got = {(p["b"]["steps"], p["b"]["v2"], p["b"]["waves"]) for fl, p in plans16 if p["b"]["kind"] in (hb.KIND_KSM1, hb.KIND_KSM2)}
  assert got == variants                                     # ... and on the B side
  # the two-pass fallback for each of its reasons: kp > 8192, k % 4 odd, a pointer off its boundary with k % 4 == 0
  fallback = [p for fl, p in plans16 if p["a"]["kind"] == hb.KIND_KSM2]
  assert any(p["kp"] > 8192 and p["a"]["vec"] for p in fallback) and any(p["kp"] <= 64 for p in fallback)
  assert any(al & 15 and k % 4 == 0 and hb.describe(1, m, n, k, fl, al, tile)["a"]["kind"] == hb.KIND_KSM2
             for f16, m, n, k, fl, al, tile in hb.products() if f16)
  assert {p["big"] for _, p in plans16} == {0, 1}           # both tile kernels
  # the row-per-wave prep of the small kernel with and without the multiplier, with and without 16-byte loads
  assert {(fl & hb.AMUL, p["a"]["vec"]) for fl, p in plans16 if p["a"]["kind"] == hb.KIND_ROWS} == {(0, 0), (0, 1), (hb.AMUL, 0), (hb.AMUL, 1)}
  # transposed operands (column passes) in both image layouts, with one and with many slabs, B with the multiplier
  for side, flag in (("a", hb.AT), ("b", 0)):
    cols = [(fl, p) for fl, p in plans16 if p[side]["kind"] == hb.KIND_COLS]
    assert {(p["kb"] == 16, p["nslab"] > 1) for _, p in cols} == {(False, False), (False, True), (True, False), (True, True)}, side
    assert {p[side]["vec"] for _, p in cols} == {0, 1}
  assert {p["kb"] == 16 for fl, p in plans16 if fl & hb.BMUL and p["b"]["kind"] == hb.KIND_COLS} == {False, True}
  # f16 split-K: even and ragged last slices, ragged tiles, every tail of the reduction
  split = [p for _, p in plans16 if p["slices"] > 1]
  assert any(p["last"] == p["kt_per"] for p in split) and any(p["last"] < p["kt_per"] for p in split)
  assert {p["count"] % 4 for p in split} >= {0, 2, 3} and any(p["mp"] > 256 and p["np"] > 256 for p in split)
  assert any(fl & hb.AT for fl, p in plans16 if p["slices"] > 1) and any(fl & hb.BMUL for fl, p in plans16 if p["slices"] > 1)
  # f32 split-K: both sides of K = 2048, even and ragged last slices, three slices and more
  assert any(p["slices"] == 1 and fl & hb.AT for fl, p in plans32) and any(p["slices"] > 1 for _, p in plans32)
  split = [p for _, p in plans32 if p["slices"] > 1]
  assert any(p["last"] == p["kper"] for p in split) and any(p["last"] < p["kper"] for p in split)
  assert any(p["used"] == 3 for p in split) and any(p["used"] >= 4 for p in split)
  assert any(fl & hb.BMUL for fl, p in plans32 if p["slices"] > 1)
  # 16-byte loads of the f32 kernel on and off, for both reasons
  for side, ld in (("a_vec", lambda m, n, k, fl: m if fl & hb.AT else k), ("b_vec", lambda m, n, k, fl: k if fl & hb.BT else n)):
    why = set()
    for f16, m, n, k, fl, al, tile in hb.products():
      if not f16:
        low = al & 15 if side == "a_vec" else (al >> 4) & 15
        why.add((hb.describe(0, m, n, k, fl, al)[side], ld(m, n, k, fl) % 4 == 0, low == 0))
    assert why >= {(1, True, True), (0, False, True), (0, True, False)}, (side, why)
    assert {ld(m, n, k, fl) % 4 for f16, m, n, k, fl, al, tile in hb.products() if not f16} >= {0, 1, 2}


def test_what_the_split_rule_does_for_a_single_tile():
  """Recorded in DESIGN.md: ``eff > best + 0.02`` with eff = slices / 256 for one tile keeps an earlier count until six
  more slices fit, so a single tile is not split below K = 12288 and then grows in steps of six."""
  assert [hb.g16_splits(129, 131, k) for k in (8192, 10240, 12287, 12288, 14336, 24575, 24576, 36864, 262144)] == \
      [1, 1, 1, 6, 6, 6, 12, 18, 126]
  # two tiles: eff = 2 slices / 256, so a count is kept until three more fit
  assert [hb.g16_splits(512, 256, k) for k in (8192, 12288, 14336, 16384, 65536, 131072)] == [3, 6, 6, 6, 30, 63]
  assert hb.g16_splits(3456, 3456, 65536) == 9 and hb.g16_splits(5888, 5888, 65536) == 1


# ------------------------------------------------------------------------------------------ the builders
def test_cut_lists():
  assert hb.k_cuts(1) == [0] and hb.k_cuts(13) == [0, 1, 11, 12]
  c = hb.all_cuts(129, 131, 12289)                                 # f16: 6 slices of 129 K steps; f32: 12 of 1040 rows
  assert {0, 12288, 129 * 16 - 1, 129 * 16, 5 * 129 * 16, 1040 - 1, 1040, 11 * 1040, 255, 256, 12287} <= set(c)
  assert hb.slice_cuts(1, 129, 131, 12289) == [2064 * s for s in range(1, 6)]
  assert hb.slice_cuts(0, 129, 131, 2049, hb.AT) == [1040] and hb.slice_cuts(0, 129, 131, 2047, hb.AT) == []


def _is_int_operand(a):
  return bool(np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 1023)


def _check_images(rows, want_lo_zero):
  """numpy float16 restating g16_scale_of and the split: hi + lo is the scaled value, exactly."""
  sv, hi, lo = hb.split_hi_lo(rows)
  mx = np.abs(sv).max(axis=1)
  assert np.all((mx == 0) | ((mx >= 512) & (mx < 1024)))
  assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), sv.astype(np.float64))
  assert np.isfinite(hi.astype(np.float32)).all()
  if want_lo_zero:
    assert not lo.any()
  else:
    assert np.count_nonzero(lo) > lo.size // 2                            # the lo plane is exercised
    bits = np.abs(sv[sv != 0].astype(np.float64)) * 2.0 ** 12
    assert np.array_equal(bits, np.rint(bits)) and (np.log2(bits.max()) > 21)   # 22 significant bits: more than fp16's 11


def _product_cases():
  out = [("scores16", (m, n, k), tile) for m, n, k, tile, _, _ in hb.SCORES16]
  out += [("dense16", (m, n, k), tile) for m, n, k, tile, *_ in hb.DENSE_FWD16]
  out += [("fwd32", s, 0) for s in hb.FWD32]
  return sorted(set(out))


@pytest.mark.parametrize("family", ["int", "sel_a", "sel_b"])
def test_products_are_exact(family):
  for name, (m, n, k), tile in _product_cases():
    c = hb.product(family, m, n, k, hb.case_rng("host", family, m, n, k), tile)
    a, b = c["a"], c["b"]
    assert a.shape == (m, k) and b.shape == (k, n) and a.dtype == b.dtype == np.float32
    assert hb.exact_f32(c["ref"]) and np.array_equal(c["ref"], hb.f64(a) @ hb.f64(b))
    small = m * k + n * k < 3 << 20
    if family == "int":
      assert _is_int_operand(a) and _is_int_operand(b)
      assert c["terms"] + 50 < hb.EXACT_BOUND                              # (the largest bias is 50)
      ref64 = a.astype(np.int64) @ b.astype(np.int64)
      assert np.array_equal(ref64, c["ref"])
      if m > 2 and n > 2:
        assert not a[m // 2].any() and not b[:, n // 2].any()              # a zero row and a zero column
        assert len({float(v) for v in np.abs(a).max(axis=1)}) >= 3          # the scales differ
      cuts = hb.all_cuts(m, n, k, tile)
      assert a[0, cuts].all() and a[m - 1, cuts].all() or m > 2 and m // 2 in (0, m - 1)     # planted next to every cut
      assert np.all(a[0, 0::16] != 0) and np.all(a[0, 15::16] != 0)
      if small:
        _check_images(a, True)
        _check_images(np.ascontiguousarray(b.T), True)
    else:
      dense, sel = (a, b) if family == "sel_b" else (np.ascontiguousarray(b.T), np.ascontiguousarray(a.T))
      assert np.count_nonzero(sel, axis=0).max() <= 1 and set(np.unique(sel)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
      out = c["ref"] if family == "sel_b" else c["ref"].T
      src, val = c["src"], c["val"]
      live = np.flatnonzero(src >= 0)
      assert np.array_equal(out[:, live], hb.f64(dense)[:, src[live]] * hb.f64(val[live]))
      cuts = [x for x in hb.all_cuts(m, n, k, tile)]
      assert set(src[live]) >= set(cuts[:: max(1, len(cuts) // max(1, len(live) - 1))][:1])     # the planted sources lead
      if small:
        _check_images(dense, False)
        _check_images(np.ascontiguousarray(sel.T), True)


@pytest.mark.parametrize("case", hb.CROSS_FWD16 + [(b, d, 0) for b, d in hb.CROSS_FWD32], ids=str)
def test_cross_forward_cases_are_exact(case):
  batch, d, tile = case
  for act in (False, True):
    c = hb.cross_fwd_case(batch, d, hb.case_rng("host", case), tile, act)
    assert c["terms"] < hb.EXACT_BOUND and c["diag"] in (0.25, 0.5)
    assert all(_is_int_operand(c[name]) for name in ("x0", "x", "w", "bias"))
    assert all(hb.exact_f32(c[name]) for name in ("pre", "u", "y"))
    assert np.array_equal(c["pre"], c["x"].astype(np.int64) @ c["w"].astype(np.int64) + c["bias"].astype(np.int64))
    assert np.array_equal(c["y"] * 4, np.rint(c["y"] * 4))               # multiples of 0.25
    _check_images(c["x"], True)
    _check_images(np.ascontiguousarray(c["w"].T), True)


@pytest.mark.parametrize("case", hb.CROSS_BWD16 + [(b, d, 0) for b, d in hb.CROSS_BWD32] +
                         [(c, 1, 0) for c in hb.MUL_COUNTS] + [hb.BIG_MUL + (0,)], ids=str)
def test_cross_backward_cases_are_exact(case):
  batch, d, tile = case
  c = hb.cross_bwd_case(batch, d, hb.case_rng("host", case), tile)
  assert c["terms"] < hb.EXACT_BOUND and c["diag"] in (0.25, 0.5)
  dz = c["dy"].astype(np.int64) * c["x0"].astype(np.int64)
  assert np.array_equal(dz, c["dz"]) and _is_int_operand(c["dz"])          # after the fused multiplier: |v| <= 1023
  assert np.abs(c["dy"]).max() <= 3 and np.abs(c["x0"]).max() > 3 and not c["x0"].all() or d == 1
  assert all(_is_int_operand(c[name]) for name in ("x", "w", "bias", "add", "dy"))
  assert all(hb.exact_f32(c[name]) for name in ("u", "dx0", "dx", "dw", "db"))
  assert np.array_equal(c["dw"], c["x"].astype(np.int64).T @ dz) and np.array_equal(c["db"], dz.sum(axis=0))
  assert hb.exact_f32(c["dx0"] + hb.f64(c["add"]) + c["dx"])
  if batch * d < 1 << 20 and d * d < 1 << 22:
    _check_images(c["dz"], True)
    _check_images(np.ascontiguousarray(c["dz"].T), True)
    _check_images(c["w"], True)


@pytest.mark.parametrize("family", ["int", "sel"])
@pytest.mark.parametrize("case", hb.DENSE_BWD16 + [c + (0,) for c in hb.DENSE_BWD32], ids=str)
def test_dense_backward_cases_are_exact(case, family):
  batch, din, dout, tile = case
  c = hb.dense_bwd_case(family, batch, din, dout, hb.case_rng("host", family, case), tile)
  assert all(hb.exact_f32(c[name]) for name in ("dx", "dw"))
  if family == "int":
    assert c["terms"] < hb.EXACT_BOUND and all(_is_int_operand(c[name]) for name in ("x", "w", "dy", "add"))
    assert hb.exact_f32(c["db"]) and hb.exact_f32(c["dx_add"])
    assert np.array_equal(c["dw"], c["x"].astype(np.int64).T @ c["dy"].astype(np.int64))
  else:
    assert np.count_nonzero(c["w"], axis=1).max() <= 1 and np.count_nonzero(c["x"], axis=0).max() <= 1
    _check_images(c["dy"], False)                                          # rows of dy: the dx product
    _check_images(np.ascontiguousarray(c["dy"].T), False)                  # columns of dy: the dW product
    _check_images(c["w"], True)
    _check_images(np.ascontiguousarray(c["x"].T), True)
