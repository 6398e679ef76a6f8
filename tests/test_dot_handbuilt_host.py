"""The hand-built DotInteraction inputs of tests/dot_handbuilt.py, proved on the host: the exactness conditions are
derived again from the arrays alone, a set of deliberately wrong restatements shows that the inputs can tell a subtly
wrong kernel from a right one, and the route every case of tests/test_dot_layout_gpu.py is named for is asked from the
library's own decision function (``tfrs_dot_interaction_plan``: what the launchers switch on), enumerated over the
whole shape grid.  No GPU access: the plan entry points do no device work."""

import ctypes

import numpy as np
import pytest

from recommenders_amd import _lib
from tests import dot_handbuilt as hb

KIB = 1024


# ------------------------------------------------------------------------------------------ the plan entry
def test_plan_entry_point_rejects_bad_arguments():
  lib, out = _lib.load(), (ctypes.c_int64 * 32)()
  for args in [(0, 5, 5, 0, 0, 0), (5, 0, 5, 0, 0, 0), (5, 5, 0, 0, 0, 0), (-1, 5, 5, 0, 0, 0), (5, 5, 16, 0, 1, 1)]:
    assert lib.tfrs_dot_interaction_plan(*args, out) == _lib.TFRS_EINVAL, args
  assert lib.tfrs_dot_interaction_plan(5, 5, 5, 0, 0, 0, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_dot_interaction_plan_many(1, None, None) == _lib.TFRS_EINVAL
  assert lib.tfrs_dot_interaction_plan_many(0, None, None) == _lib.TFRS_OK
  p = hb.plan(67, 33, 64, True)
  assert hb.route_name("fwd", p["fwd"]) == "fwd.f16x3_direct<64,2,3>" and hb.route_name("bwd", p["bwd"]) == "bwd.dense<2,12>"
  assert (p["fwd"]["grid"], p["fwd"]["threads"], p["fwd"]["lds"]) == (17, 256, 0)
  row = hb.plan_many([(67, 33, 64, 1, 0, 0)])[0]
  assert [int(v) for v in row[:16]] == list(p["fwd"].values()) and [int(v) for v in row[16:]] == list(p["bwd"].values())


def test_the_benchmark_shape_keeps_its_kernels():
  """B = 131072, F = 101, D = 32 runs the producer / consumer forward and the split-fp16 backward,
  contiguous and strided."""
  for strided in (0, 1):
    p = hb.plan(131072, 101, 32, False, False, strided)
    assert hb.route_name("fwd", p["fwd"]) == "fwd.pc<4,4>" and (p["fwd"]["grid"], p["fwd"]["lds"]) == (512, 75248)
    assert hb.route_name("bwd", p["bwd"]) == "bwd.h16<7,5,4>" and (p["bwd"]["grid"], p["bwd"]["threads"]) == (256, 512)


# ------------------------------------------------------------------------------------------ exactness
def _unique_cases():
  seen, out = set(), []
  for c in hb.all_cases():
    if c.shape_row()[:5] not in seen:
      seen.add(c.shape_row()[:5])
      out.append(c)
  return out


def _seven_bits(a):
  """Every entry of the group (last axes flattened) is an integer multiple of 2^(floor(log2 max) - 6): seven mantissa
  bits relative to the largest, so fp16's eleven hold it under any power-of-two scale that keeps the largest finite."""
  a = np.abs(np.asarray(a, np.float64)).reshape(a.shape[0], -1)
  mx = a.max(axis=1)
  unit = np.exp2(np.floor(np.log2(np.where(mx > 0, mx, 1.0))) - 6)
  q = a / unit[:, None]
  return bool(np.array_equal(q, np.rint(q)))


def _hi_exact_lo_zero(a):
  """numpy float16 restating the split: scaled so that the group's largest lies in [2^12, 2^13), hi is the value."""
  a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
  mx = np.abs(a).max(axis=1)
  k = np.where(mx > 0, 12 - np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 0)
  sv = a * np.exp2(k)[:, None]
  hi = sv.astype(np.float16)
  return bool(np.isfinite(hi.astype(np.float32)).all() and np.array_equal(hi.astype(np.float64), sv))


@pytest.mark.parametrize("case", _unique_cases(), ids=str)
def test_cases_are_exact(case):
  c = case.build()
  x, dy, b, f = c["x"], c["dy"], case.batch, case.f
  assert x.dtype == dy.dtype == np.float32 and x.shape == (b, f, case.d) and dy.shape == (b, case.n)
  assert np.abs(c["m"]).max() <= hb.MAX_M and np.abs(c["mdy"]).max(initial=0) <= hb.MAX_M
  assert np.abs(c["eb"]).max() <= hb.E_RANGE and np.abs(c["edy"]).max() <= hb.E_RANGE
  assert c["gi"].min() >= 0 and c["gi"].max() <= hb.G_RANGE
  assert np.array_equal(x, c["m"] * np.exp2(c["eb"][:, None, None] + c["gi"][None, :, None]))
  assert np.array_equal(dy, c["mdy"] * np.exp2(c["edy"][:, None]))
  # the sum of |terms| of every entry, in units of the sample's common scale, is an integer below 2^24
  tf, tb = hb.term_sums(x, dy, case.self_i, case.skip)
  uf = tf / np.exp2(2.0 * c["eb"])[:, None]
  ub = tb / np.exp2(c["eb"] + c["edy"])[:, None, None]
  assert np.array_equal(uf, np.rint(uf)) and np.array_equal(ub, np.rint(ub))
  assert uf.max(initial=0) < hb.EXACT_BOUND and ub.max(initial=0) < hb.EXACT_BOUND
  # seven mantissa bits relative to the largest, per sample and per 32-row block; hi exact, lo zero
  groups = [x, dy] + [x[:, r: r + 32] for r in range(0, f, 32)]
  assert all(_seven_bits(g) and _hi_exact_lo_zero(g) for g in groups if g.size)
  # the float64 results are float32 values and are what the oracle computes
  # (the oracle on the first samples, which hold everything planted: its einsum is slow and every sample runs the same code)
  k = min(b, 12)
  for name, ref in (("out", hb.oracle_forward(x[:k], case.self_i, case.skip)),
                    ("dx", hb.oracle_backward(x[:k], dy[:k], case.self_i, case.skip))):
    assert np.array_equal(c[name].astype(np.float32).astype(np.float64), c[name]), name
    assert np.array_equal(c[name][:k].reshape(ref.shape), ref.astype(np.float64)), name
  # what is planted
  p = hb.planted(b, f)
  assert not x[p["zero_x"]].any() and not dy[p["zero_dy"]].any()
  sample, row = p["zero_row"]
  assert not x[sample, row].any() and (f == 1 or x[sample].any())
  if (f + 31) // 32 > 1:
    sample, blk = p["zero_block"]
    assert not x[sample, 32 * blk: 32 * blk + 32].any() and x[sample, : 32 * blk].any()
  live = [s for s in range(b) if s not in (p["zero_x"], p["zero_row"][0], p["zero_block"][0])]
  assert np.all(np.abs(x[live]).max(axis=2) > 0)                       # no other zero row
  assert len(set(c["eb"])) > 3 and c["eb"].max() == hb.E_RANGE and c["eb"].min() == -hb.E_RANGE


# ------------------------------------------------------------------------------------------ sensitivity
def test_wrong_restatements_differ_on_every_case_they_apply_to():
  counts = dict.fromkeys(("offset", "pad", "stale", "diagonal", "rows", "upper", "noself"), 0)
  for case in _unique_cases():
    if case.n == 0:
      continue
    c = case.build()
    x, dy, f, d, self_i, skip = c["x"], c["dy"], case.f, case.d, case.self_i, case.skip
    ref, dref = c["out"], c["dx"]

    def differs(name, got, want=ref):
      counts[name] += 1
      assert got.shape == want.shape and not np.array_equal(got, want), (name, case)

    if not skip and f >= (2 if self_i else 3):
      differs("offset", hb.mutant_previous_row_offset(x, self_i))
    if 0 < hb.padded(d) != d and (f >= 3 or (self_i and f >= 2)):
      differs("pad", hb.mutant_pad_from_next_feature(x, self_i, skip))
    plan = case.planned()
    for direction, want in (("fwd", ref), ("bwd", dref)):
      r = plan[direction]
      if r["kernel"] in hb.PERSISTENT and hb.samples_per_trip(r) < case.batch:
        differs("stale", hb.mutant_stale_sample(want, hb.samples_per_trip(r)), want)
    if self_i:
      differs("diagonal", hb.backward64(x, dy, self_i, skip, double_diagonal=False), dref)
    if not skip and f % 32 and f >= 2:
      got, guard = hb.mutant_rows_past_f_stored(x, self_i)
      assert guard
      differs("rows", got)
    if skip and f >= 2:
      differs("upper", hb.mutant_upper_not_zeroed(x))
    if not self_i and f >= 2:
      differs("noself", hb.mutant_noself_diagonal(x, skip))
  assert all(v >= 10 for v in counts.values()), counts


# ------------------------------------------------------------------------------------------ the whole grid
F_GRID = D_GRID = range(1, 141)
BATCHES = (1, 511, 512)
SWITCH_SETTINGS = [(s, f, None) for s in hb.STAGE_VALUES for f in hb.FWD_VALUES] + \
                  [(None, None, b) for b in hb.BWD_VALUES[1:]] + [("0", "staged", "gather"), (None, "f32", "pc")]


def _grid_rows():
  rows = [(b, f, d, s, k, st) for b in BATCHES for s in (0, 1) for k, st in ((0, 0), (1, 0), (0, 1))
          for f in F_GRID for d in D_GRID]
  return np.asarray(rows, np.int64)


@pytest.fixture(scope="module")
def grid():
  """{switch setting: (rows, plans)} over F, D in 1..140, both triangles, skip_gather, strided, batch 1 / 511 / 512."""
  rows = _grid_rows()
  out = {}
  for sw in SWITCH_SETTINGS:
    with hb.switches(*sw):
      out[sw] = hb.plan_many(rows)
  return rows, out


def _distinct_routes(plans, direction, variants=False):
  """The distinct (kernel, template arguments) of one half of the plans, as names (variants: hb.variant_name)."""
  whole = plans[:, :16] if direction == "fwd" else plans[:, 16:]
  half = whole[:, :10]
  key = np.zeros(len(half), np.int64)
  if variants:
    key = np.where(whole[:, 0] == hb.GATHER, whole[:, 15], 0) * 2 + (whole[:, 13] > 80 * KIB) * (whole[:, 0] == hb.FWD_PC)
    assert key.min() >= 0 and key.max() < 10
  for col, radix in enumerate((16, 129, 5, 2, 4, 5, 34, 9, 9, 5)):      # one more than the largest value of the column
    assert half[:, col].min() >= 0 and half[:, col].max() < radix
    key = key * radix + half[:, col]
  _, first = np.unique(key, return_index=True)
  name = hb.variant_name if variants else hb.route_name
  return {name(direction, list(whole[i])) for i in first}


def test_every_reachable_route_has_a_case_and_every_case_its_route(grid):
  rows, plans = grid
  reachable = set()
  for sw, p in plans.items():
    reachable |= _distinct_routes(p, "fwd") | _distinct_routes(p, "bwd")
  reachable -= {"fwd.refused", "bwd.refused"}
  named = {c.route for c in hb.ROUTE_CASES}
  assert sorted(reachable - named) == [], "routes without a case"
  assert sorted(named - reachable) == [], "cases named for a route nothing reaches"
  assert len(reachable) == 101                                          # (said in DESIGN.md section 2)
  # what the decision varies without a template argument (the fallback backward's 4 / 2 / 1 samples per workgroup, the
  # 160 KiB request of the producer / consumer forward past 80 KiB of LDS) is held by the route cases as well
  variants, have = set(), set()
  for sw, p in plans.items():
    variants |= _distinct_routes(p, "fwd", True) | _distinct_routes(p, "bwd", True)
  for c in hb.ROUTE_CASES:
    have.add(hb.variant_name(c.direction, c.planned()[c.direction]))
  assert sorted(v for v in variants - have if "refused" not in v) == [] and len(variants - reachable - {"fwd.refused", "bwd.refused"}) == 4
  assert {"bwd.gather/4", "bwd.gather/2", "bwd.gather/1", "fwd.pc<4,4>/160K"} <= have
  for c in hb.all_cases():
    p = c.planned()
    assert hb.route_name(c.direction, p[c.direction]) == c.route, c
    # both directions run on the GPU, but for the backward routes that exist only where the forward is refused
    assert p["bwd"]["kernel"] != hb.REFUSED, c
    assert p["fwd"]["kernel"] != hb.REFUSED or c.route in ("bwd.dense<4,20>", "bwd.dense<4,33>") or \
        hb.variant_name("bwd", p["bwd"]) == "bwd.gather/1", c
  # the shapes of the route list follow the rule it states
  for c in hb.ROUTE_CASES:
    assert c.batch in (hb.SMALL, hb.LARGE) and not c.strided
  for (route, f, d, self_i, sw) in hb.GRID_STRIDE:
    c, g = hb.grid_stride_case(route, f, d, self_i, sw)
    assert c.batch == 2 * g + 5 and hb.samples_per_trip(c.planned()[c.direction]) == g
    assert g == c.planned()[c.direction]["grid"] * (4 if "direct" in route else 1)
    assert c.batch * f * max(d, f) * 4 < 100 << 20                      # well under 100 MB


def test_forward_accepted_means_backward_accepted(grid):
  rows, plans = grid
  for sw, p in plans.items():
    fwd, bwd = p[:, 0], p[:, 16]
    bad = rows[(fwd != hb.REFUSED) & (bwd == hb.REFUSED)]
    assert len(bad) == 0, (sw, bad[:5])


def test_strided_supported_is_both_strided_plans(grid):
  rows, plans = grid
  q = _lib.load().tfrs_dot_interaction_strided_supported
  for sw, p in plans.items():
    strided = rows[:, 5] == 1
    ok = (p[:, 0] != hb.REFUSED) & (p[:, 16] != hb.REFUSED) & strided
    # the query on EVERY strided row of the grid, accepted or refused
    want = ok.tolist()
    with hb.switches(*sw):
      for i in np.flatnonzero(strided).tolist():
        b, f, d, s = rows[i, :4].tolist()
        assert q(b, f, d, s) == want[i], (sw, b, f, d, s)
    if sw == (None, None, None):
      acc = rows[ok]
      assert set(acc[:, 2]) == {16, 32} and set(acc[:, 0]) == {512} and acc[:, 1].max() == 122
      assert len(acc) == 2 * 2 * 122 - 2            # (F = 1 without self interaction has no pairs to fuse)


def test_planned_lds_fits_the_limit_the_launcher_requests(grid):
  rows, plans = grid
  for sw, p in plans.items():
    for off in (0, 16):
      kernel, lds, limit = p[:, off], p[:, off + 12], p[:, off + 13]
      assert set(np.unique(limit)) <= {0, 64 * KIB, 80 * KIB, 160 * KIB}
      asks = limit > 0
      assert np.all(lds[asks] <= limit[asks]) and np.all(lds[~asks] <= 64 * KIB)
      assert np.all(lds[kernel <= hb.NONE] == 0)
      grid_sz, threads = p[:, off + 10], p[:, off + 11]
      run = kernel > hb.NONE
      assert np.all((grid_sz[run] >= 1) & (grid_sz[run] <= np.maximum(rows[run, 0], 1)) & (threads[run] % 64 == 0))
  # the producer / consumer forward asks for one workgroup per CU where two row images pass 80 KiB
  assert hb.plan(512, 108, 32)["fwd"]["lds_limit"] == 80 * KIB and hb.plan(512, 109, 32)["fwd"]["lds_limit"] == 160 * KIB
  assert hb.plan(512, 128, 32, True)["fwd"]["lds"] == 100880


def _forward_refused(f, d):
  """DESIGN.md section 2, as inequalities."""
  dp = hb.padded(d)
  resident = f <= 128 and d <= 128 and -(-f // 32) * (dp // 2) <= 128
  return not resident and f * (d + 1) > 4096


def _backward_refused(f, d):
  return (f > 128 or d > 128) and f * d > 16384


def test_the_refused_region_is_the_documented_one(grid):
  rows, plans = grid
  contiguous = rows[:, 5] == 0
  want_f = np.asarray([_forward_refused(int(f), int(d)) for f, d in rows[:, 1:3]])
  want_b = np.asarray([_backward_refused(int(f), int(d)) for f, d in rows[:, 1:3]])
  for sw, p in plans.items():
    assert np.array_equal((p[:, 0] == hb.REFUSED)[contiguous], want_f[contiguous]), sw
    assert np.array_equal((p[:, 16] == hb.REFUSED)[contiguous], want_b[contiguous]), sw
  for (f, d), accepted in hb.ENVELOPE_EDGES.items():
    for self_i in (0, 1):
      assert (hb.plan(67, f, d, self_i)["fwd"]["kernel"] != hb.REFUSED) == accepted, (f, d)
      assert _forward_refused(f, d) == (not accepted)
  for b, f, d, self_i, skip in hb.REFUSED_CASES:
    assert hb.plan(b, f, d, self_i, skip)["fwd"]["kernel"] == hb.REFUSED
  # no pairs: nothing to launch in either direction
  for d in (1, 32, 140):
    p = hb.plan(67, 1, d)
    assert p["fwd"]["kernel"] == p["bwd"]["kernel"] == hb.NONE
    assert hb.plan(67, 1, d, True)["fwd"]["kernel"] > hb.NONE and hb.plan(67, 1, d, False, True)["fwd"]["kernel"] > hb.NONE
