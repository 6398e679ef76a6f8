"""The hand-built batches of tests/softmax_handbuilt.py, proved on the host: every property a case of
tests/test_softmax_layout_gpu.py relies on is derived again from the arrays alone, in float64, and the split geometry
each case claims is asked from the library's own planners (``tfrs_inbatch_softmax_plan_f32`` / ``_plan_f16``, the
functions the launches call) under the options the GPU test sets.  No GPU access: the plan entry points do no device
work.

The last tests document the gap this file closes: on every shape the suite had for the f32 kernels a wave streams
exactly one tile per split, and the split-fp16 backward never met a multiple of 3 above 1 in its 3-deep ring nor an odd
count of 3 or more in its 2-deep ring."""

import ctypes

import numpy as np
import pytest

from recommenders_amd import _lib
from tests import softmax_handbuilt as hb


class options:
  """``with options(TFRS_SOFTMAX_WAVES="1"): ...`` -- set through tfrs_set_option, always restored to None."""

  def __init__(self, **kw):
    self.kw = {k: v for k, v in kw.items() if v is not None}

  def __enter__(self):
    for k, v in self.kw.items():
      _lib.set_option(k, v)

  def __exit__(self, *exc):
    for k in self.kw:
      _lib.set_option(k, None)


def lib_plan_f32(nq, heads, nc):
  out = (ctypes.c_int64 * 4)()
  _lib.check(_lib.load().tfrs_inbatch_softmax_plan_f32(nq, heads, nc, out))
  return list(out)


def lib_plan_f16(nq, nc):
  out = (ctypes.c_int64 * 6)()
  _lib.check(_lib.load().tfrs_inbatch_softmax_plan_f16(nq, nc, out))
  return list(out)


def test_plan_entry_points_reject_bad_arguments():
  out = (ctypes.c_int64 * 6)()
  lib = _lib.load()
  assert lib.tfrs_inbatch_softmax_plan_f32(0, 1, 5, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f32(5, 33, 5, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f32(6, 1, 5, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f32(5, 1, 5, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f16(0, 5, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f16(6, 5, out) == _lib.TFRS_EINVAL
  assert lib.tfrs_inbatch_softmax_plan_f16(5, 5, None) == _lib.TFRS_EINVAL


def test_planner_targets_are_read_on_every_call():
  base32, base16 = lib_plan_f32(97, 1, 97), lib_plan_f16(97, 97)
  assert base32 == [4, 32, 4, 32] and base16 == [4, 32, 4, 32, 4, 32]
  with options(TFRS_SOFTMAX_WAVES="1", TFRS_SOFTMAX_WGS="1"):
    assert lib_plan_f32(97, 1, 97) == [1, 128, 1, 128]
    assert lib_plan_f16(97, 97) == [1, 128, 4, 32, 4, 32]
    with options(TFRS_SOFTMAX_WGS_BWD="2"):
      assert lib_plan_f16(97, 97) == [1, 128, 2, 64, 2, 64]
  assert lib_plan_f32(97, 1, 97) == base32 and lib_plan_f16(97, 97) == base16


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("waves,heads,shape,fwd,dc", hb.F32_DEPTH_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_f32_depth_cases_have_the_claimed_geometry(waves, heads, shape, fwd, dc):
  nq, nc, _ = shape
  with options(TFRS_SOFTMAX_WAVES=waves):
    got = lib_plan_f32(nq, heads, nc)
  assert got == hb.plan_f32(nq, heads, nc, waves)
  assert hb.split_tiles(nc, got[0], got[1]) == fwd
  assert hb.split_tiles(nq * hb.padded_heads(heads), got[2], got[3]) == dc
  assert max(fwd[0]) >= 2, "the forward / dq wave streams several tiles"


def test_f32_depth_case_with_the_last_positive_alone_in_the_ragged_tile():
  nq, nc = 97, 97
  assert (nq - 1) // hb.TILE == 3 and nc - 3 * hb.TILE == 1      # row 96's positive is the only row of tile 3


# ------------------------------------------------------------------------------------------ B
def _assert_no_probability_in_the_flush_band(s):
  """exp(s - rowmax) is a normal float32 (with room: >= 2^-120) or rounds to 0 in float32 (< 2^-150)."""
  z = s - s.max(axis=1, keepdims=True)
  assert not np.any((z < -120 * np.log(2.0)) & (z > -150 * np.log(2.0)))


@pytest.mark.parametrize("step", hb.STAIR_STEPS)
@pytest.mark.parametrize("kind", hb.STAIR_KINDS)
def test_staircases_put_every_rows_maximum_where_they_say(kind, step):
  nq, nc, d = hb.STAIR_SHAPE
  q, c, levels, t = hb.staircase(nq, nc, d, kind, step)
  assert np.all(np.abs(q[:, 1:]) <= 0.5) and np.all(np.abs(c[:, 1:]) <= 0.5)
  assert np.all(q * 4 == np.round(q * 4)) and np.all(c * 4 == np.round(c * 4)) and np.abs(c).max() <= 64
  # no exact 0 beside nonzero entries of the same coordinate: no gradient entry is made of flushed terms only
  assert np.all(c[:, 1:] != 0) and np.all(q[:, :1 + hb.STAIR_NOISE] != 0) and np.all(q[:, 1 + hb.STAIR_NOISE:] == 0)
  inv_t = np.float32(1.0) / np.float32(t)
  assert float(inv_t) == 1.0 / t and np.log2(float(inv_t)) % 1 == 0           # a power of two: the logits stay exact
  s = hb.logits64(q, c, t)
  assert np.array_equal(s.astype(np.float32).astype(np.float64), s)           # ... in float32
  _assert_no_probability_in_the_flush_band(s)
  tm = hb.tile_maxima(s)
  assert tm.shape == (nq, 6)
  order = np.argsort(levels, kind="stable")
  for lo, hi in zip(order[:-1], order[1:]):
    if levels[hi] > levels[lo]:
      assert np.all(tm[:, hi] - tm[:, lo] >= step), (kind, step, lo, hi)
  assert np.all(tm.argmax(axis=1) == int(np.argmax(levels)))
  if kind == "ascending":
    assert np.all(np.diff(tm, axis=1) >= step)               # the rescale fires on every tile
  if kind == "descending":
    assert np.all(np.diff(tm, axis=1) <= -step)              # ... and never after the first
  gaps = np.concatenate([np.abs(tm[:, i] - tm[:, j]) for i in range(6) for j in range(i)
                         if abs(levels[i] - levels[j]) == 1])      # between tiles one level apart
  if step == 8:
    assert np.exp(-gaps.max()) > 2.0 ** -24                  # the previous tile still contributes
  if step >= 40:
    assert np.exp(-gaps.min()) < 2.0 ** -24                  # earlier sums fall below an ulp of the new one
  if step >= 120:
    assert np.float32(np.exp(-gaps.min())) == 0.0 and -gaps.min() * np.log2(np.e) < -149   # 0 on the base-2 path too


def test_staircase_geometry_on_both_paths():
  nq, nc, _ = hb.STAIR_SHAPE
  with options(TFRS_SOFTMAX_WAVES="1", TFRS_SOFTMAX_WGS="1", TFRS_SOFTMAX_WGS_BWD="1"):
    p32, p16 = lib_plan_f32(nq, 1, nc), lib_plan_f16(nq, nc)
  assert hb.split_tiles(nc, *p32[:2]) == ([6], 1) and hb.split_tiles(nc, *p16[:2]) == ([6], 1)
  assert hb.split_tiles(nc, *p16[2:4]) == ([6], 1)
  # default options: every tile a split of its own -- the maximum moves between splits, the finalize kernels combine
  assert hb.split_tiles(nc, *lib_plan_f32(nq, 1, nc)[:2])[0] == [1] * 6
  assert hb.split_tiles(nc, *lib_plan_f16(nq, nc)[:2])[0] == [1] * 6


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("nw", ("4", "8"))
def test_f16_depth_shapes_have_the_claimed_tiles_and_cover_every_ring_residue(nw):
  seen = {(depth, side): set() for depth in (2, 3) for side in ("dq", "dc")}
  guard = {2: set(), 3: set()}                   # (t + NB - 1 < nt) per tile, as a tuple: last true / first false
  for (nq, nc), (ft, ct) in hb.F16_DEPTH_SHAPES.items():
    with options(TFRS_SOFTMAX_WGS="1", TFRS_SOFTMAX_WGS_BWD="1", TFRS_SOFTMAX_NW=nw):
      got = lib_plan_f16(nq, nc)
    assert got == hb.plan_f16(nq, nc, nw, 1, 1)
    assert hb.split_tiles(nc, *got[:2])[0] == [ft] and hb.split_tiles(nc, *got[2:4])[0] == [ft]
    assert hb.split_tiles(nq, *got[4:])[0] == [ct]
    for depth in (2, 3):
      seen[depth, "dq"].add(ft % depth)
      seen[depth, "dc"].add(ct % depth)
      for nt in (ft, ct):
        guard[depth].add(tuple(t + depth - 1 < nt for t in range(nt)))
  for (depth, side), residues in seen.items():
    assert residues == set(range(depth)), (depth, side, residues)
  assert any(n % 3 == 0 and n > 3 for n, _ in hb.F16_DEPTH_SHAPES.values())          # a multiple of 3 above 1 round
  assert any(n % 2 == 1 and n >= 3 for pair in hb.F16_DEPTH_SHAPES.values() for n in pair)
  for depth in (2, 3):                           # the prefetch guard is true on all but the last depth - 1 tiles
    assert all(g.count(False) == min(depth - 1, len(g)) for g in guard[depth])
  assert [hb.ring_depth(d) for d in hb.F16_DEPTH_DIMS] == [3, 3, 2]
  assert (192 % hb.TILE, 192 // hb.TILE) == (0, 6)                                  # the row without a ragged tile


def test_f16_two_split_shapes():
  for (nq, nc), (ft, ct) in hb.F16_TWO_SPLIT_SHAPES.items():
    with options(TFRS_SOFTMAX_WGS="2", TFRS_SOFTMAX_WGS_BWD="2"):
      got = lib_plan_f16(nq, nc)
    assert got == hb.plan_f16(nq, nc, None, 2, 2)
    assert hb.split_tiles(nc, *got[:2])[0] == ft and hb.split_tiles(nc, *got[2:4])[0] == ft
    assert hb.split_tiles(nq, *got[4:])[0] == ct


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("shape,nsplit", list(hb.FINALIZE_SHAPES.items()), ids=lambda v: str(v).replace(" ", ""))
def test_finalize_shapes_split_per_tile_and_the_planted_split_holds_the_maximum(shape, nsplit):
  nq, nc, d = shape
  got = lib_plan_f16(nq, nc)
  assert got == hb.plan_f16(nq, nc) and got[:2] == [nsplit, 32]
  assert nsplit >= 16 and (nsplit > 16) == (nc > 512)
  for at in hb.finalize_plants(nsplit):
    q, c, _, t = hb.staircase(nq, nc, d, at, hb.FINALIZE_GAP)
    _assert_no_probability_in_the_flush_band(hb.logits64(q, c, t))
    tm = hb.tile_maxima(hb.logits64(q, c, t))                  # one tile per split: the split maxima
    assert np.all(tm.argmax(axis=1) == at)
    others = np.delete(tm, at, axis=1)
    assert np.all(tm[:, at] - others.max(axis=1) >= hb.FINALIZE_GAP)


# ------------------------------------------------------------------------------------------ E
def _tile_max_abs(g, axis_rows):
  """max |G| per streamed tile for every owned row: [owned, tiles]."""
  g = np.abs(g if axis_rows else g.T)
  return hb.tile_maxima(g)


def test_dq_ladder_rows_climb_at_least_three_binades_per_tile():
  nq, nc, d = 161, 161, 16
  q, c, _, _ = hb.staircase(nq, nc, d, "ascending")
  _assert_no_probability_in_the_flush_band(hb.logits64(q, c))
  tm = _tile_max_abs(hb.softmax_g(q, c), True)                 # owned query x candidate tile
  late = np.arange(128, nq)                                    # positives in tiles 4 and 5: four climbing tiles before
  ratio = tm[late, 1:4] / tm[late, 0:3]
  assert np.all(ratio >= 2.0 ** 3), ratio.min()
  q, c, _, _ = hb.staircase(nq, nc, d, "descending")
  tm = _tile_max_abs(hb.softmax_g(q, c), True)
  late = np.arange(64, nq)                                     # positives behind the first two tiles
  assert np.all(tm[late, 1:2] / tm[late, 0:1] <= 2.0 ** -3)


@pytest.mark.parametrize("ascending", (True, False))
def test_column_ladder_climbs_on_the_dc_side(ascending):
  nq, nc, d = 129, 161, 16
  q, c, below = hb.column_ladder(nq, nc, d, ascending)
  assert np.all(q * 4 == np.round(q * 4)) and np.all(c * 4 == np.round(c * 4)) and np.abs(q).max() <= 8
  assert np.all(c[:, 1:] != 0) and np.all(q[:, 1:1 + hb.STAIR_NOISE] != 0) and np.all(q[:, 1 + hb.STAIR_NOISE:] == 0)
  _assert_no_probability_in_the_flush_band(hb.logits64(q, c))
  tm = _tile_max_abs(hb.softmax_g(q, c), False)[list(hb.LADDER_LIKED)]       # liked candidate x query tile
  assert tm.shape == (3, 5)
  ratio = tm[:, 1:] / tm[:, :-1]
  # 2^8 per tile: the 2^3 the issue asks for, times the 2^5 that the per-record scale of the streamed queries (largest
  # |q| of a tile: 8 .. 0.5) may take back
  assert np.all(ratio >= 2.0 ** 8) if ascending else np.all(ratio <= 2.0 ** -8), ratio


# ------------------------------------------------------------------------------------------ the gap, documented
def test_existing_f32_shapes_never_stream_a_second_tile():
  for nq, nc in hb.F32_EXISTING_SHAPES:
    got = lib_plan_f32(nq, 1, nc)
    assert got == hb.plan_f32(nq, 1, nc)
    assert set(hb.split_tiles(nc, *got[:2])[0]) == {1} and set(hb.split_tiles(nq, *got[2:])[0]) == {1}
  got = lib_plan_f32(4096, 1, 4096)                            # ... while the benchmark's shape runs 16 splits of 8
  assert got == hb.plan_f32(4096, 1, 4096) and hb.split_tiles(4096, *got[:2])[0] == [8] * 16


def test_existing_f16_backward_depths_miss_ring_residues():
  counts = hb.F16_EXISTING_BWD_TILES
  assert not any(n % 3 == 0 for n in counts if n > 1)          # 3-deep ring: no multiple of 3
  # 2-deep ring (d > 64): the suite's shapes at d = 100 and 128 give 1 and 2 tiles per split only
  with_d = {(300, 4500): 100, (100, 333): 100, (1024, 1024): 128, (257, 300): 128, (64, 97): 128}
  for (nq, nc), d in with_d.items():
    got = lib_plan_f16(nq, nc)
    assert got == hb.plan_f16(nq, nc)
    assert hb.ring_depth(d) == 2
    for n_stream, plan in ((nc, got[2:4]), (nq, got[4:])):
      assert set(hb.split_tiles(n_stream, *plan)[0]) <= {1, 2}
