"""The hand-built optimizer cases of tests/optimizer_handbuilt.py without a GPU: every property a builder claims to plant
is asserted again from the arrays alone, and the cases are shown to be SENSITIVE -- a kernel that contracted a product
into the sum behind it, or added the squares of a row in another order, would change the bits that
tests/test_optimizer_layout_gpu.py compares."""

import numpy as np
import pytest

from tests import clippy_restatement as crs
from tests import optimizer_handbuilt as hb
from tests import rowwise_adagrad_restatement as rw
from tests import table_optimizers_restatement as rs


def _share(a, b):
  """Fraction of the elements whose bits differ."""
  return float((hb.bits(a) != hb.bits(b)).mean())


def _normal_or_zero(arrays, label):
  for i, a in enumerate(arrays):
    a = np.asarray(a)
    assert a.dtype == np.float32, (label, i)
    assert np.isfinite(a).all(), (label, i)
    mag = np.abs(a[a != 0])
    assert not mag.size or mag.min() >= hb.MIN_NORMAL, (label, i, float(mag.min()))


def _rule_states(case):
  """(w, slots, g, alpha) before every step of a rule case."""
  w, slots = case["w"], case["slots"]
  for g, a, out in zip(case["grads"], case["alphas"], case["ref"]):
    yield w, slots, g, a
    w, slots = out["w"], out["slots"]


# ---- the rules ------------------------------------------------------------------------------------------------------------
def test_rule_hyper_parameters():
  """The five ``rs.RULES`` entries; only SGD's learning rate differs (0.3 is no power of two, the suite's 256 is)."""
  assert hb.RULE_NAMES == ("adam", "ftrl", "ftrl_power0", "ftrl_reg", "sgd")
  for name in hb.RULE_NAMES:
    kind, hp = hb.rule_hyper(name)
    assert kind == rs.RULES[name][0]
    if kind == "SGD":
      assert hp == dict(learning_rate=0.3)
      assert np.log2(float(np.float32(0.3))) % 1 != 0 and np.log2(rs.SGD_LR) % 1 == 0
    else:
      assert hp == rs.RULES[name][1]
  h = hb.rule_hyper_floats(*hb.rule_hyper("ftrl_reg"))
  assert h.dtype == np.float32 and h.shape == (8,) and h[4] == -0.5 and h[1] == np.float32(1e-5)
  assert hb.rule_hyper_floats(*hb.rule_hyper("ftrl_power0"))[4] == 0.0


@pytest.mark.parametrize("name", hb.RULE_NAMES)
def test_rule_cases_keep_every_intermediate_normal_or_zero(name):
  """Every intermediate of the float32 restatement -- ``rule_intermediates`` computes them all and ends on the bits of
  ``rs.update`` -- is finite and either 0 or at least 2^-126 in magnitude, on the 32-tensor list, on a small tensor and
  on the sparse cases' summed gradients: the comparison does not depend on how subnormals are handled.  Ftrl's ``linear``
  is never exactly 0 after a step (where it is, the sign of clip(lin) - lin depends on which zero a max returns)."""
  kind, hp = hb.rule_hyper(name)
  cases = [hb.list_rule_case(name, hb.LIST_32)[0], hb.rule_case(name, 5)]
  for case in cases:
    for w, slots, g, a in _rule_states(case):
      _normal_or_zero([w, g] + list(slots), name)
      out = hb.rule_intermediates(kind, w, slots, g, hp, a)
      ref = rs.update(kind, w, slots, g, hp, np.float32, alpha=a)
      assert np.array_equal(hb.bits(out["w"]), hb.bits(ref["w"]))
      for x, y in zip(out["slots"], ref["slots"]):
        assert np.array_equal(hb.bits(x), hb.bits(y))
      _normal_or_zero(out["all"], name)
      if kind == "Ftrl":
        assert (out["lin2"] != 0).all()
  for route, vocab, dims in (("rowscan", hb.ROWSCAN_VOCAB, hb.SPARSE_DIMS), ("sorted", hb.SORTED_VOCAB, hb.SPARSE_DIMS_SORTED)):
    ids_case = hb.sparse_ids(vocab, np.int64)
    for d in dims:
      rows = hb.sparse_rows(ids_case, d)
      uniq, g = rs.sum_duplicates(ids_case["ids"], rows, vocab, rs.piece_length(d) if route == "sorted" else None)
      rng = np.random.default_rng(d)
      w = hb.rule_weights(rng, (vocab, d))
      slots, t0 = hb.rule_start(name, rng, w)
      out = hb.rule_intermediates(kind, w[uniq], [s[uniq] for s in slots], g, hp, hb.rule_alpha(name, t0))
      _normal_or_zero([g] + out["all"], (name, route, d))
      if kind == "Ftrl":
        assert (out["lin2"] != 0).all()


def test_the_suites_own_cases_keep_every_intermediate_normal_or_zero():
  """The condition above is one the project's randomized cases already meet: it can be met."""
  for name in hb.RULE_NAMES:
    kind, hp = rs.RULES[name]
    sizes, ws, grads = rs.dense_case(name, steps=1)
    w, g = np.concatenate(ws), np.concatenate(grads[0])
    slots = rs.initial_slots(kind, hp, w)
    out = hb.rule_intermediates(kind, w, slots, g, hp, rs.adam_alpha(hp, 1) if kind == "Adam" else None)
    _normal_or_zero(out["all"], name)


def test_fused_variants_differ_from_the_restatement():
  """The sensitivity of the rule cases: the fused variant of every rule changes the bits of at least 5 % of the elements
  of at least one output.  (With the suite's SGD_LR = 256 the product lr * g is exact and NO element changes.)"""
  shares = {}
  for name in hb.RULE_NAMES:
    kind, hp = hb.rule_hyper(name)
    case = hb.list_rule_case(name, hb.LIST_32)[0]
    w, slots, g, a = next(_rule_states(case))
    ref = case["ref"][0]
    fused = hb.fused_update(kind, w, slots, g, hp, a)
    share = dict(w=_share(fused["w"], ref["w"]))
    for key, x, y in zip(rs.SLOTS[kind], fused["slots"], ref["slots"]):
      share[key] = _share(x, y)
    shares[name] = share
    assert max(share.values()) >= 0.05, (name, share)
  print("fused shares", shares)
  assert shares["sgd"]["w"] >= 0.05
  assert shares["adam"]["m"] >= 0.05 and shares["adam"]["v"] >= 0.05
  assert all(shares[n]["accumulator"] >= 0.05 for n in ("ftrl", "ftrl_reg", "ftrl_power0"))
  case = hb.list_rule_case("sgd", hb.LIST_32)[0]
  at_256 = dict(learning_rate=rs.SGD_LR)
  fused = hb.fused_update("SGD", case["w"], [], case["grads"][0], at_256)
  assert _share(fused["w"], rs.update("SGD", case["w"], [], case["grads"][0], at_256, np.float32)["w"]) == 0.0


def test_fused_variants_equal_the_restatement_where_nothing_rounds():
  """The fused variants are the same formulas: on inputs whose products are exact they give the restatement's bits."""
  rng = np.random.default_rng(3)
  w = (rng.integers(-8, 9, size=500) * 2.0 ** -4).astype(np.float32)
  g = (rng.choice([-1.0, 1.0], size=500) * 2.0 ** rng.integers(-3, 1, size=500)).astype(np.float32)
  hp = dict(learning_rate=0.5)
  assert _share(hb.fused_update("SGD", w, [], g, hp)["w"], rs.update("SGD", w, [], g, hp, np.float32)["w"]) == 0.0
  hp = dict(learning_rate=1.0, beta_1=0.5, beta_2=0.75, epsilon=0.0)
  m, v = g * np.float32(0.5), g * g * np.float32(0.25)
  fused, ref = hb.fused_update("Adam", w, [m, v], g, hp, 0.5), rs.update("Adam", w, [m, v], g, hp, np.float32, alpha=0.5)
  assert _share(fused["w"], ref["w"]) == 0.0 and _share(fused["slots"][0], ref["slots"][0]) == 0.0
  assert _share(fused["slots"][1], ref["slots"][1]) == 0.0


# ---- the sum of squares ---------------------------------------------------------------------------------------------------
def test_kernel_order_sum_of_squares_by_hand():
  """d = 8, VEC = 4: two chunks on two lanes, ((g0^2 + g1^2) + g2^2) + g3^2 plus the same of the second chunk.  d = 8,
  VEC = 1: eight lanes of one square, a tree of three levels that pairs l with l ^ 4, then ^ 2, then ^ 1.  d = 130 on the
  row scan: lanes 0 and 1 hold three squares, the rest two."""
  g = np.array([[3.0, 1e-4, 7.0, 2e-4, 5.0, 3e-4, 11.0, 4e-4]], dtype=np.float32)
  sq = (g * g)[0]
  chunk = lambda c: ((sq[4 * c] + sq[4 * c + 1]) + sq[4 * c + 2]) + sq[4 * c + 3]
  assert hb.group_lanes(8, 4) == 2 and hb.group_lanes(8, 1) == 8
  assert hb.bits(hb.sum_squares_kernel_order(g, 4))[0] == hb.bits(chunk(0) + chunk(1))
  tree = ((sq[0] + sq[4]) + (sq[2] + sq[6])) + ((sq[1] + sq[5]) + (sq[3] + sq[7]))
  assert hb.bits(hb.sum_squares_kernel_order(g, 1))[0] == hb.bits(tree)
  assert [hb.group_lanes(d, 1) for d in (1, 2, 3, 5, 63, 64, 65, 257)] == [1, 2, 4, 8, 64, 64, 64, 64]
  assert [hb.group_lanes(d, 4) for d in (4, 8, 200, 256, 260, 520)] == [1, 2, 64, 64, 64, 64]
  wide = hb.rowwise_case(3, 130)[2] + np.float32(1e-3)
  sq = wide * wide
  partial = sq[:, :64] + sq[:, 64:128]
  partial[:, :2] = partial[:, :2] + sq[:, 128:130]
  assert np.array_equal(hb.bits(hb.sum_squares_rowscan_order(wide)), hb.bits(hb._butterfly(partial)))


def test_kernel_order_differs_from_the_other_orders():
  """On 500 rows of d = 200 the kernel order (VEC = 4) differs from ``sequential`` in at least half of the rows, and
  VEC = 4 from VEC = 1 in at least a tenth.  The row scan's order and the VEC = 1 order are the SAME sum at every width
  up to 256: with one feature per chunk lane l owns l, l + 64, ... on both, and lanes without a feature add +0."""
  g = (np.random.default_rng(200).normal(size=(500, 200)) * 3e-3).astype(np.float32)
  seq = rw._sum_squares(g, "sequential")
  v4, v1 = hb.sum_squares_kernel_order(g, 4), hb.sum_squares_kernel_order(g, 1)
  shares = dict(v4_seq=_share(v4, seq), v1_seq=_share(v1, seq), v4_v1=_share(v4, v1))
  print("order shares", shares)
  assert shares["v4_seq"] >= 0.5 and shares["v1_seq"] >= 0.5 and shares["v4_v1"] >= 0.1
  assert _share(v4, rw._sum_squares(g, "pairwise")) >= 0.1
  for d in (1, 3, 5, 63, 64, 65, 200, 256):
    x = (np.random.default_rng(d).normal(size=(50, d)) * 3e-3).astype(np.float32)
    assert np.array_equal(hb.bits(hb.sum_squares_rowscan_order(x)), hb.bits(hb.sum_squares_kernel_order(x, 1)))
  # every order is the same number up to rounding
  exact = (g.astype(np.float64) ** 2).sum(axis=1)
  for s in (seq, v4, v1):
    assert np.allclose(s, exact, rtol=201 * 2.0 ** -24, atol=0)


def test_update_takes_the_sum_it_is_given():
  """``rw.update(..., sum_sq=...)``: the sequential sum passed in gives the bits of ``order="sequential"`` (whose results
  are unchanged), the kernel order gives other accumulators on most rows, and all-zero gradient rows keep their bits."""
  w, acc, g = hb.rowwise_case(67, 200)
  hp = rw.hyper(learning_rate=hb.ROWWISE_LR)
  a = rw.update(w, acc, g, hp, np.float32)
  b = rw.update(w, acc, g, hp, np.float32, sum_sq=rw._sum_squares(g, "sequential"))
  assert np.array_equal(hb.bits(a["w"]), hb.bits(b["w"])) and np.array_equal(hb.bits(a["acc"]), hb.bits(b["acc"]))
  c = rw.update(w, acc, g, hp, np.float32, sum_sq=hb.sum_squares_kernel_order(g, 4))
  zero = (g == 0).all(axis=1)
  assert zero.sum() == 13 and list(np.flatnonzero(zero)[:2]) == [4, 9]
  assert np.array_equal(hb.bits(c["w"][zero]), hb.bits(w[zero])) and np.array_equal(hb.bits(c["acc"][zero]), hb.bits(acc[zero]))
  assert (hb.bits(c["w"][~zero]) != hb.bits(w[~zero])).mean() > 0.9
  # the order of the sum is visible in the RESULTS of the row-wise case, not only in the sum: the accumulators start below
  # the rows' mean square gradient.  (From the suite's 0.025 .. 0.225 every order gives the same accumulator.)
  c1 = rw.update(w, acc, g, hp, np.float32, sum_sq=hb.sum_squares_kernel_order(g, 1))
  shares = dict(v4_seq=_share(c["acc"][~zero], a["acc"][~zero]), v4_v1=_share(c["acc"][~zero], c1["acc"][~zero]),
                w_v4_seq=_share(c["w"][~zero], a["w"][~zero]))
  print("row-wise result shares", shares)
  assert shares["v4_seq"] >= 0.5 and shares["v4_v1"] >= 0.1 and shares["w_v4_seq"] >= 0.25
  big = (acc * np.float32(1e5)).astype(np.float32)
  assert _share(rw.update(w, big, g, hp, np.float32, sum_sq=hb.sum_squares_kernel_order(g, 4))["acc"],
                rw.update(w, big, g, hp, np.float32)["acc"]) == 0.0
  with pytest.raises(AssertionError):
    rw.update(w, acc, g, hp, np.float32, sum_sq=np.zeros(67))       # (float64 sums for a float32 step)


def test_rowwise_dims_reach_every_instantiation():
  """per_row = 1, idle lanes in a group, REREAD on the scalar path from d = 65 and on the float4 path from d = 260; the
  grid cap of the dense kernel."""
  paths = {d: hb.rowwise_path(d, True) for d in hb.ROWWISE_DIMS}
  assert {p for p in paths.values()} == {(4, False), (4, True), (1, False), (1, True)}
  assert paths[64] == (4, False) and paths[65] == (1, True) and paths[63] == (1, False) and paths[1] == (1, False)
  assert paths[256] == (4, False) and paths[260] == (4, True) and paths[520] == (4, True) and paths[257] == (1, True)
  assert {hb.rowwise_path(d, False) for d in hb.ROWWISE_DIMS} == {(1, False), (1, True)}
  assert hb.rowwise_path(64, False) == (1, False) and hb.rowwise_path(200, False) == (1, True)
  assert hb.group_lanes(4, 4) == 1 and hb.group_lanes(1, 1) == 1                 # per_row = 1
  assert hb.group_lanes(5, 1) == 8 and hb.group_lanes(200, 4) == 64              # 3 and 14 idle lanes
  rows = 65_600
  assert -(-(rows * hb.group_lanes(256, 4)) // 256) > hb.ROWWISE_GRID_CAP >= -(-(65_536 * 64) // 256)


# ---- the dense layouts ----------------------------------------------------------------------------------------------------
def test_dense_lists_hold_what_the_issue_names():
  lists = hb.dense_lists()
  assert hb.DENSE_SIZES == (0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, 13315)
  assert [lists[f"n{n}"] for n in hb.DENSE_SIZES] == [(n,) for n in hb.DENSE_SIZES]
  l32 = lists["list32"]
  assert len(l32) == 32 and l32[0] == 0 and l32[-1] == 0 and set(l32) == set(hb.DENSE_SIZES)
  empties = [k for k, n in enumerate(l32) if n == 0]
  assert empties == [0, 9, 10, 31]
  assert set(lists["all_empty"]) == {0}
  assert len(lists) == len(hb.DENSE_SIZES) + 2


def test_packed_buffers_are_guarded_and_aligned_as_named():
  for alignment in hb.ALIGNMENTS:
    for op in hb.OPERANDS:
      off = hb.operand_off(alignment, op)
      offsets, total = hb.pack(hb.LIST_32, off)
      assert total % 4 == 0
      end = 0
      for o, n in zip(offsets, hb.LIST_32):
        if n == 0:
          assert o is None
          continue
        assert o % 4 == (1 if off else 0) and o - end >= hb.GUARD
        end = o + n
      assert total - end >= hb.GUARD
  assert [hb.operand_off("s0_off", op) for op in hb.OPERANDS] == [False, True, False, False]
  assert all(hb.operand_off("all_off", op) for op in hb.OPERANDS)
  assert not any(hb.operand_off("aligned", op) for op in hb.OPERANDS)
  flat = hb.packed((3, 0, 5), True, [np.ones(3, np.float32), None, np.full(5, 2, np.float32)])
  offsets, total = hb.pack((3, 0, 5), True)
  assert offsets == [9, None, 21] and total == 40 and flat.size == 40
  assert (flat == hb.SENTINEL).sum() == 40 - 8 and flat[9:12].tolist() == [1, 1, 1] and flat[21:26].tolist() == [2] * 5


def test_dense_layouts_reach_both_paths_a_block_end_and_a_double_advance():
  """``first_block`` and the float4 / scalar choice restated from (sizes, alignment): over the lists both paths, a tensor
  that ends exactly on a block, the scalar path on a FULL block (one operand 4 bytes off) and a walk that passes one and
  two empty tensors all occur; every block is owned by a non-empty tensor (an empty tensor's pointers are never read)."""
  seen = set()
  for lname, sizes in hb.dense_lists().items():
    for alignment in hb.ALIGNMENTS:
      offs = [hb.operand_off(alignment, op) for op in hb.OPERANDS]
      lay = hb.dense_blocks(sizes, offs)
      fb = lay["first_block"]
      assert len(fb) == len(sizes) + 1 and fb[-1] == sum(-(-n // hb.DENSE_BLOCK) for n in sizes)
      covered = [np.zeros(n, np.int64) for n in sizes]
      prev_k = -1
      for b, (k, base, path, over_empty) in enumerate(lay["blocks"]):
        n = sizes[k]
        assert n > 0 and fb[k] <= b < fb[k + 1] and 0 <= base < n
        covered[k][base:min(n, base + hb.DENSE_BLOCK)] += 1
        full = base + hb.DENSE_BLOCK <= n
        assert path == ("float4" if full and alignment == "aligned" else "scalar")
        seen.add(path)
        if full and path == "scalar":
          seen.add("full_block_scalar:" + alignment)
        if full and base + hb.DENSE_BLOCK == n:
          seen.add("ends_on_a_block")
        if not full:
          seen.add("ending_block")
        if k != prev_k:                      # the first block of a tensor: how many empty tensors the walk passed last
          gap = k - prev_k - 1
          assert all(sizes[j] == 0 for j in range(prev_k + 1, k))
          seen.add(f"passes_{gap}_empty")
          prev_k = k
        assert over_empty == sum(1 for j in range(k) if sizes[j] == 0)
      assert all((c == 1).all() for c in covered)             # every element in exactly one block
      if fb[-1] == 0:
        seen.add("no_launch:" + lname)
  want = {"float4", "scalar", "ends_on_a_block", "ending_block", "passes_0_empty", "passes_1_empty", "passes_2_empty",
          "no_launch:n0", "no_launch:all_empty"} | {"full_block_scalar:" + a for a in hb.ALIGNMENTS if a != "aligned"}
  assert seen == want, seen ^ want
  # a double advance between two CONSECUTIVE blocks: block 8 belongs to tensor 8, block 10 to tensor 11
  lay = hb.dense_blocks(hb.LIST_32, [False] * 4)
  owners = [k for k, _, _, _ in lay["blocks"]]
  assert any(b - a == 3 for a, b in zip(owners[:-1], owners[1:])) and owners[0] == 1
  assert hb.tensor_walk(lay["first_block"], 32, lay["first_block"][11]) == (11, 3)


# ---- exact cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,eps", hb.ADAGRAD_EXACT)
def test_adagrad_exact_cases_are_exact(mode, eps):
  """float64, float32 and fused float32 evaluation agree bit for bit, the step moves every element with a gradient, and
  on the eps != 0 cases the other mode gives different results."""
  assert np.float32(eps) == eps
  for n in (5, 4097, 13315):
    c = hb.adagrad_exact_case(n, mode, eps)
    w64, a64 = hb.adagrad_eval(c["w"], c["acc"], c["g"], c["lr"], eps, mode, np.float64)
    w32, a32 = hb.adagrad_eval(c["w"], c["acc"], c["g"], c["lr"], eps, mode, np.float32)
    wf, af = hb.adagrad_eval(c["w"], c["acc"], c["g"], c["lr"], eps, mode, np.float32, fused=True)
    assert w32.dtype == np.float32 and a32.dtype == np.float32 and np.isfinite(w64).all()
    assert np.array_equal(w64, w32.astype(np.float64)) and np.array_equal(a64, a32.astype(np.float64))
    assert np.array_equal(hb.bits(w64.astype(np.float32)), hb.bits(w32)) and np.array_equal(hb.bits(wf), hb.bits(w32))
    assert np.array_equal(hb.bits(a64.astype(np.float32)), hb.bits(a32)) and np.array_equal(hb.bits(af), hb.bits(a32))
    moved = c["g"] != 0
    assert (w32[moved] != c["w"][moved]).all() and np.array_equal(hb.bits(w32[~moved]), hb.bits(c["w"][~moved]))
    other, _ = hb.adagrad_eval(c["w"], c["acc"], c["g"], c["lr"], eps, 3 - mode, np.float64)
    if eps == 0.0:
      assert np.array_equal(other, w64)
      assert n < 100 or ((~moved).sum() >= 100 and len(set(np.abs(w32 - c["w"])[moved])) == 4)    # steps lr / {1, 2, 4, 8}
    else:
      assert (other != w64).all()


@pytest.mark.parametrize("mode", hb.CLIPPY_MODES)
def test_clippy_exact_cases_are_exact_and_their_factors_as_planted(mode):
  """Every tensor of every list: the factor is exactly the planted 2^-j, or exactly 1; float64, float32 and the fused
  float32 evaluation agree bit for bit in weights, accumulators and factor; exactly one element is clipped where one is
  planted and none elsewhere."""
  hp = hb.clippy_exact_hyper(mode)
  for key in ("learning_rate", "variable_relative_threshold", "accumulator_relative_threshold", "absolute_threshold"):
    assert np.log2(hp[key]) % 1 == 0
  assert crs._mode(hp) == mode and hp["epsilon"] == 0.0
  places = set()
  for lname, (sizes, plants) in hb.clippy_lists().items():
    assert len(sizes) == len(plants)
    for k, (n, plant) in enumerate(zip(sizes, plants)):
      if n == 0:
        assert plant is None
        continue
      w, acc, g = hb.clippy_exact_tensor(n, mode, plant, seed=k)
      r64, r32, rf = crs.update(w, acc, g, hp, np.float64), crs.update(w, acc, g, hp, np.float32), hb.clippy_fused(w, acc, g, hp)
      want = 1.0 if plant is None else 2.0 ** -plant[1]
      assert float(r64["factor"]) == want and float(r32["factor"]) == want and float(rf["factor"]) == want, (lname, k)
      for key in ("w", "acc"):
        assert np.array_equal(r64[key], r32[key].astype(np.float64)), (lname, k, key)
        assert np.array_equal(hb.bits(rf[key]), hb.bits(r32[key])), (lname, k, key)
      clipped = np.flatnonzero(np.abs(r64["delta"]) > r64["maxd"])
      assert clipped.tolist() == ([] if plant is None else [plant[0]]), (lname, k)
      if plant is not None:
        assert np.abs(r64["delta"][plant[0]]) == 2.0 ** plant[1] * r64["maxd"][plant[0]]
        if len(sizes) == 1:
          places.add(lname.split(".")[1])
      if n >= 100:
        assert (r32["w"] != w).mean() > 0.9 and (mode == 2 or (r32["acc"] != acc).mean() > 0.9)
  assert places == {"first", "last_full", "tail", "last"}


def test_clippy_plants_of_the_list_of_32():
  """Seven planted tensors with distinct j at all four kinds of place; one between two unclipped tensors, one beside an
  empty tensor, one beside another planted tensor; every size alone at every place it offers."""
  sizes, plants = hb.clippy_lists()["list32"]
  planted = {k: p for k, p in enumerate(plants) if p is not None}
  assert sorted(planted) == sorted(hb.LIST_32_PLANTS) and len({j for _, j in planted.values()}) == 7
  assert {place for place, _ in hb.LIST_32_PLANTS.values()} == {"first", "last_full", "tail", "last"}
  kind = lambda k: "empty" if sizes[k] == 0 else ("planted" if k in planted else "one")
  around = {k: (kind(k - 1), kind(k + 1)) for k in planted}
  assert around[7] == ("one", "one") and around[1] == ("empty", "one") and around[30] == ("one", "empty")
  assert around[12] == ("planted", "planted") and around[11][0] == "empty"
  assert hb.plant_positions(4097) == dict(first=0, last_full=4095, last=4096)
  assert hb.plant_positions(13315) == dict(first=0, last_full=12287, tail=12287 + 1 + 513, last=13314)
  assert hb.plant_positions(1) == dict(first=0) and hb.plant_positions(3) == dict(first=0, tail=1, last=2)
  assert hb.plant_positions(4096) == dict(first=0, last_full=4095, last=4095)
  singles = [name for name in hb.clippy_lists() if name.startswith("n") and not name.endswith(".none")]
  assert len(singles) == sum(len(hb.plant_positions(n)) for n in hb.DENSE_SIZES)


# ---- sparse cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("vocab", [hb.ROWSCAN_VOCAB, hb.SORTED_VOCAB])
def test_sparse_ids_hold_what_they_claim(vocab, id_dtype):
  case = hb.sparse_ids(vocab, id_dtype)
  ids = case["ids"]
  assert ids.dtype == id_dtype and ids.size <= 400 and vocab % 4 == (1 if vocab == 37 else 0)
  wide = ids.astype(np.int64)
  valid = wide[(wide >= 0) & (wide < vocab)]
  counts = np.bincount(valid, minlength=vocab)
  assert counts[hb.HOT_ID] >= hb.HOT_COUNT > rs.piece_length(8) and counts[case["zero_pair"]] == 2
  assert counts[0] >= 1 and counts[vocab - 1] >= 1 and (counts[case["untouched"]] == 0).all()
  assert (counts > 1).sum() >= 10                              # duplicates beside the hot id
  for bad in (-1, vocab, hb.INT32_MAX):
    assert (wide == bad).sum() == 3
  assert (wide == hb.WRAPS_TO_3).sum() == (3 if id_dtype == np.int64 else 0)
  for d in (1, 8):
    rows = hb.sparse_rows(case, d)
    for piece in (None, rs.piece_length(d)):
      uniq, g = rs.sum_duplicates(ids, rows, vocab, piece)
      at = int(np.flatnonzero(uniq == case["zero_pair"])[0])
      assert (g[at] == 0).all()
      if d == 8:                                    # (at d = 1 a planted zero gradient is a whole row)
        assert (np.abs(g).sum(axis=1) > 0).sum() == uniq.size - 1
  if id_dtype == np.int64:
    assert np.array_equal(hb.sparse_ids(vocab, np.int32)["untouched"], case["untouched"])
  perm = hb.unique_ids(vocab, id_dtype)
  assert perm.dtype == id_dtype and np.array_equal(np.sort(perm), np.arange(vocab)) and (np.diff(perm) != 1).any()
