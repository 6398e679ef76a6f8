"""The optimizer kernels (csrc/table_update.hip, csrc/clippy.hip, the rule kernels at the end of csrc/sparse_update.hip)
on hand-built tensors and rows (tests/optimizer_handbuilt.py, proved on the host by
tests/test_optimizer_handbuilt_host.py), through the C entry points, compared BIT FOR BIT.

  a. tfrs_table_update_dense_multi: the five rules over every dense list (each size alone, 32 tensors with empty ones
     first, last and twice in the middle, an all-empty list) and every alignment variant, two consecutive steps from the
     kernel's own state, against ``table_optimizers_restatement.update(..., np.float32)``.
  b. tfrs_table_update_sparse: both routes, int32 and int64 ids, touched rows against the restatement on the route's
     summed gradient, untouched rows and their slots unchanged.
  c. tfrs_adagrad_dense_multi and tfrs_clippy_dense_multi (compiled with contraction on) on inputs where every operation
     is exact, against float64; every Clippy factor exactly as planted.
  d. tfrs_rowwise_adagrad_dense / _sparse against ``rowwise_adagrad_restatement.update(..., np.float32)`` with the sum of
     squares in the order of the path taken (VEC 4 or 1 x REREAD, or the row scan).
  e. The same update through the dense kernel, the sorted route and the row scan: the same bits.

Every buffer a kernel may write is a slice of a larger one filled with a sentinel that must survive; the whole buffer is
compared, sentinels included.  No comparison has a tolerance.  Left out: the device-learning-rate instantiations
(tests/test_lr_schedules_gpu.py holds them to these kernels bit for bit) and the non-temporal variants (tables above
1 GiB)."""

import ctypes

import numpy as np
import pytest

from tests import clippy_restatement as crs
from tests import optimizer_handbuilt as hb
from tests import rowwise_adagrad_restatement as rw
from tests import table_optimizers_restatement as rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32


def _lib():
  from recommenders_amd import _lib
  return _lib


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _same(got, want, label):
  """Whole buffers, sentinels included, bit for bit; the message tells a write outside a tensor from a wrong value."""
  got, want = hb.bits(got.detach().cpu().numpy()), hb.bits(want)
  if not np.array_equal(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    outside = int((want.reshape(-1)[bad] == hb.bits(hb.SENTINEL)).sum())
    raise AssertionError(f"{label}: {bad.size} of {got.size} elements differ, {outside} of them sentinels "
                         f"(first at {int(bad[0])})")


class Packed:
  """One operand of a dense multi-tensor call: the tensors of ``arrays`` inside ONE flat device buffer of sentinels
  (``hb.pack``), an empty tensor as a NULL pointer."""

  def __init__(self, sizes, off, arrays):
    self.sizes, self.off = sizes, off
    self.offsets, _ = hb.pack(sizes, off)
    self.dev = _dev(hb.packed(sizes, off, arrays))
    assert self.dev.data_ptr() % 16 == 0
    base = self.dev.data_ptr()
    self.ptrs = (ctypes.c_void_p * len(sizes))(*[None if o is None else base + 4 * o for o in self.offsets])
    for p, n in zip(self.ptrs, sizes):
      assert (p is None) == (n == 0) and (p is None or p % 16 == (4 if off else 0))

  def check(self, arrays, label):
    _same(self.dev, hb.packed(self.sizes, self.off, arrays), label)


def _sizes_arg(sizes):
  return (ctypes.c_int64 * len(sizes))(*sizes)


def _guarded(a):
  """(flat device buffer, view of ``a``'s shape inside it, 16-byte aligned, with sentinels on either side)."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  pad = 64 + 4 * (a.shape[-1] if a.ndim == 2 else 0)
  flat = np.full((a.size + 2 * pad,), hb.SENTINEL, dtype=np.float32)
  flat[pad:pad + a.size] = a.reshape(-1)
  dev = _dev(flat)
  view = dev[pad:pad + a.size].view(a.shape)
  assert view.data_ptr() % 16 == 0
  return dev, view, pad


def _guarded_want(a, pad):
  a = np.ascontiguousarray(a, dtype=np.float32)
  flat = np.full((a.size + 2 * pad,), hb.SENTINEL, dtype=np.float32)
  flat[pad:pad + a.size] = a.reshape(-1)
  return flat


def _misaligned(a):
  """``a`` on the device as a contiguous view that starts one float into a flat buffer of sentinels: (flat, view, pad)."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  pad = 65 + 4 * (a.shape[-1] if a.ndim == 2 else 0)
  flat = np.full((a.size + 2 * pad,), hb.SENTINEL, dtype=np.float32)
  flat[pad:pad + a.size] = a.reshape(-1)
  dev = _dev(flat)
  view = dev[pad:pad + a.size].view(a.shape)
  assert view.data_ptr() % 16 == 4
  return dev, view, pad


def _workspace(nbytes):
  return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device="cuda")


def _alpha_dev(a):
  return None if a is None else torch.tensor([float(a)], dtype=torch.float32, device="cuda")


# ---- a. the rule kernel on dense tensors --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hb.RULE_NAMES)
def test_dense_rule_kernel_on_hand_built_layouts(name):
  """``table_update_dense_multi_kernel<RULE>`` on its float4 and its scalar path: every list x alignment variant, two
  steps, weights and both slots against the float32 restatement, the gradient untouched, all sentinels intact.  An empty
  tensor's pointers are NULL (never read); a call without elements returns without a launch."""
  lib = _lib()
  L = lib.load()
  kind, hp = hb.rule_hyper(name)
  hyper = (ctypes.c_float * 8)(*hb.rule_hyper_floats(kind, hp))
  nslots = len(rs.SLOTS[kind])
  calls = 0
  for lname, sizes in hb.dense_lists().items():
    case, cuts = hb.list_rule_case(name, sizes)
    split = lambda a: [a[c] for c in cuts]
    alphas = [_alpha_dev(a) for a in case["alphas"]]
    for alignment in hb.ALIGNMENTS:
      if alignment in ("s0_off", "s1_off") and not nslots:
        continue                                           # (SGD has no such operand)
      label = f"{name} {lname} {alignment}"
      p = Packed(sizes, hb.operand_off(alignment, "p"), split(case["w"]))
      slots = [Packed(sizes, hb.operand_off(alignment, op), split(s)) for op, s in zip(("s0", "s1"), case["slots"])]
      for step, (g, ref) in enumerate(zip(case["grads"], case["ref"])):
        gp = Packed(sizes, hb.operand_off(alignment, "g"), split(g))
        lib.check(L.tfrs_table_update_dense_multi(
            hb.RULE_INDEX[kind], hyper, lib.ptr(alphas[step]), len(sizes), p.ptrs, slots[0].ptrs if nslots else None,
            slots[1].ptrs if nslots else None, gp.ptrs, _sizes_arg(sizes), lib.current_stream()))
        calls += 1
        p.check(split(ref["w"]), f"{label} step {step} w")
        for s, want, key in zip(slots, ref["slots"], rs.SLOTS[kind]):
          s.check(split(want), f"{label} step {step} {key}")
        gp.check(split(g), f"{label} step {step} gradient")
  assert calls == 2 * len(hb.dense_lists()) * (len(hb.ALIGNMENTS) if nslots else len(hb.ALIGNMENTS) - 2)


# ---- b. the rule kernels on sparse rows -------------------------------------------------------------------------------------
def _sparse_rule_call(name, route, d, id_dtype, ids, rows, vocab, table, slots, alpha):
  """One ``tfrs_table_update_sparse`` step from (table, slots) on guarded buffers: (table buffer, slot buffers, pads)."""
  lib = _lib()
  L = lib.load()
  kind, hp = hb.rule_hyper(name)
  hyper = (ctypes.c_float * 8)(*hb.rule_hyper_floats(kind, hp))
  rowscan = 1 if route == "rowscan" else 0
  n = ids.size
  tb = _guarded(table)
  sb = [_guarded(s) for s in slots]
  ids_t, rows_t, alpha_t = _dev(ids), _dev(rows), _alpha_dev(alpha)
  nbytes = L.tfrs_table_update_workspace_bytes(n, rowscan)
  ws = _workspace(nbytes)
  lib.check(L.tfrs_table_update_sparse(
      hb.RULE_INDEX[kind], hyper, lib.ptr(alpha_t), lib.ptr(rows_t), lib.ptr(ids_t), 1 if id_dtype == np.int64 else 0,
      n, d, vocab, lib.ptr(tb[1]), lib.ptr(sb[0][1]) if sb else None, lib.ptr(sb[1][1]) if sb else None, rowscan,
      lib.ptr(ws), nbytes, lib.current_stream()))
  assert np.array_equal(rows_t.cpu().numpy().view(np.uint32), hb.bits(rows))
  return tb, sb


@pytest.mark.parametrize("route", ["rowscan", "sorted"])
@pytest.mark.parametrize("name", hb.RULE_NAMES)
def test_sparse_rule_kernels_on_hand_built_ids(name, route):
  """``table_update_rowscan_kernel<RULE, int32 / int64>`` (vocab 37) and ``table_update_sorted_kernel<RULE, 4 / 1>``
  (vocab 1000; d = 260 too): touched rows bit for bit the restatement on the route's summed gradient -- the row whose sum
  is exactly zero included --, untouched rows and their slots unchanged, sentinels intact."""
  kind, hp = hb.rule_hyper(name)
  vocab = hb.ROWSCAN_VOCAB if route == "rowscan" else hb.SORTED_VOCAB
  dims = hb.SPARSE_DIMS if route == "rowscan" else hb.SPARSE_DIMS_SORTED
  for d in dims:
    rng = np.random.default_rng(d)
    table = hb.rule_weights(rng, (vocab, d))
    slots, t0 = hb.rule_start(name, rng, table)
    alpha = hb.rule_alpha(name, t0)
    for id_dtype in (np.int32, np.int64):
      label = f"{name} {route} d {d} {np.dtype(id_dtype).name}"
      case = hb.sparse_ids(vocab, id_dtype)
      rows = hb.sparse_rows(case, d)
      uniq, g = rs.sum_duplicates(case["ids"], rows, vocab, rs.piece_length(d) if route == "sorted" else None)
      ref = rs.update(kind, table[uniq], [s[uniq] for s in slots], g, hp, np.float32, alpha=alpha)
      want_t = table.copy()
      want_t[uniq] = ref["w"]
      want_s = [s.copy() for s in slots]
      for s, r in zip(want_s, ref["slots"]):
        s[uniq] = r
      tb, sb = _sparse_rule_call(name, route, d, id_dtype, case["ids"], rows, vocab, table, slots, alpha)
      untouched = np.setdiff1d(np.arange(vocab), uniq)
      assert np.isin(case["untouched"], untouched).all()
      got = tb[1].cpu().numpy()
      assert np.array_equal(hb.bits(got[untouched]), hb.bits(table[untouched])), label + ": an untouched row moved"
      _same(tb[0], _guarded_want(want_t, tb[2]), label + " table")
      for (buf, _, pad), want, key in zip(sb, want_s, rs.SLOTS[kind]):
        _same(buf, _guarded_want(want, pad), f"{label} {key}")


# ---- c. the kernels compiled with contraction on, on exact inputs ---------------------------------------------------------------
ACC_ALIGNMENTS = ("aligned", "all_off", "p_off", "s0_off", "g_off")       # (three operands: s0 is the accumulator)


@pytest.mark.parametrize("mode,eps", hb.ADAGRAD_EXACT)
def test_dense_adagrad_kernel_on_exact_inputs(mode, eps):
  """``adagrad_dense_multi_kernel`` over the dense lists and alignment variants: parameters and accumulators are bit for
  bit the float64 result (every operation is exact, so a contracted multiply-add cannot differ), sentinels intact."""
  lib = _lib()
  L = lib.load()
  for lname, sizes in hb.dense_lists().items():
    cases = [hb.adagrad_exact_case(n, mode, eps, seed=k) for k, n in enumerate(sizes)]
    want = [hb.adagrad_eval(c["w"], c["acc"], c["g"], c["lr"], eps, mode, np.float64) for c in cases]
    want_w, want_a = [w.astype(np.float32) for w, _ in want], [a.astype(np.float32) for _, a in want]
    for alignment in ACC_ALIGNMENTS:
      label = f"adagrad mode {mode} eps {eps} {lname} {alignment}"
      p = Packed(sizes, hb.operand_off(alignment, "p"), [c["w"] for c in cases])
      a = Packed(sizes, hb.operand_off(alignment, "s0"), [c["acc"] for c in cases])
      g = Packed(sizes, hb.operand_off(alignment, "g"), [c["g"] for c in cases])
      lib.check(L.tfrs_adagrad_dense_multi(len(sizes), p.ptrs, a.ptrs, g.ptrs, _sizes_arg(sizes), hb.ADAGRAD_LR, eps,
                                           mode, lib.current_stream()))
      p.check(want_w, label + " w")
      a.check(want_a, label + " accumulator")
      g.check([c["g"] for c in cases], label + " gradient")


@pytest.mark.parametrize("mode", hb.CLIPPY_MODES)
def test_dense_clippy_kernels_on_exact_inputs_and_planted_factors(mode):
  """``clippy_dense_multi_kernel<false / true>``: the only clipped element of a tensor at element 0, at the end of the
  last full block, inside the ending block and at n - 1, alone and among 32 tensors.  ``factors[k]`` is exactly the
  planted 2^-j, exactly 1 for a tensor without a clipped element and for an empty one -- a neighbour's outlier leaves it
  alone --, ``factors`` beyond ``ntensors`` keep their sentinel; parameters and accumulators are bit for bit the float64
  result."""
  lib = _lib()
  L = lib.load()
  hp = hb.clippy_exact_hyper(mode)
  for lname, (sizes, plants) in hb.clippy_lists().items():
    tensors = [hb.clippy_exact_tensor(n, mode, plant, seed=k) for k, (n, plant) in enumerate(zip(sizes, plants))]
    refs = [crs.update(w, acc, g, hp, np.float64) for w, acc, g in tensors]
    want_w, want_a = [r["w"].astype(np.float32) for r in refs], [r["acc"].astype(np.float32) for r in refs]
    want_f = np.full((32 + 2 * hb.GUARD,), hb.SENTINEL, dtype=np.float32)
    want_f[hb.GUARD:hb.GUARD + len(sizes)] = [1.0 if p is None else 2.0 ** -p[1] for p in plants]
    for k, (r, n) in enumerate(zip(refs, sizes)):
      assert float(r["factor"]) == want_f[hb.GUARD + k] or n == 0
    # (a list of one tensor: the alignment variants of the three operands; the list of 32: all of them)
    for alignment in ACC_ALIGNMENTS:
      label = f"clippy mode {mode} {lname} {alignment}"
      p = Packed(sizes, hb.operand_off(alignment, "p"), [t[0] for t in tensors])
      a = Packed(sizes, hb.operand_off(alignment, "s0"), [t[1] for t in tensors])
      g = Packed(sizes, hb.operand_off(alignment, "g"), [t[2] for t in tensors])
      factors = torch.full((32 + 2 * hb.GUARD,), float(hb.SENTINEL), dtype=torch.float32, device="cuda")
      lib.check(L.tfrs_clippy_dense_multi(
          len(sizes), p.ptrs, a.ptrs, g.ptrs, _sizes_arg(sizes), ctypes.c_void_p(factors.data_ptr() + 4 * hb.GUARD),
          hp["learning_rate"], hp["epsilon"], hp["variable_relative_threshold"], hp["accumulator_relative_threshold"],
          hp["absolute_threshold"], mode, lib.current_stream()))
      _same(factors, want_f, label + " factors")
      p.check(want_w, label + " w")
      a.check(want_a, label + " accumulator")
      g.check([t[2] for t in tensors], label + " gradient")


# ---- d. RowWiseAdagrad ----------------------------------------------------------------------------------------------------
def _rowwise_hyper(mode):
  return rw.hyper(legacy=(mode == 2), learning_rate=hb.ROWWISE_LR)


def _rowwise_dense(w, acc, g, mode, aligned):
  """``tfrs_rowwise_adagrad_dense`` on guarded buffers (``aligned`` or every operand a view 4 bytes in): the buffers."""
  lib = _lib()
  hp = _rowwise_hyper(mode)
  place = _guarded if aligned else _misaligned
  wb, ab, gb = place(w), place(acc), place(g)
  rows, d = w.shape
  lib.check(lib.load().tfrs_rowwise_adagrad_dense(lib.ptr(wb[1]), lib.ptr(ab[1]), lib.ptr(gb[1]), rows, d,
                                                  hp["learning_rate"], None, hp["epsilon"], mode, lib.current_stream()))
  return wb, ab, gb


@pytest.mark.parametrize("mode", [1, 2])
def test_rowwise_dense_kernel_in_the_kernel_order(mode):
  """``rowwise_adagrad_dense_kernel<VEC, REREAD>``: d from 1 (per_row = 1) over idle lanes (3, 5, 63, 200) to REREAD on
  the scalar path (65, 257, and every d > 64 from a view 4 bytes in) and on the float4 path (260, 520); 1, 5 and 67 rows.
  Table and accumulator bit for bit the restatement with the sum of squares in the order of the path; every fifth
  gradient row is all zero and keeps its bits."""
  hp = _rowwise_hyper(mode)
  seen = set()
  for d in hb.ROWWISE_DIMS:
    for rows in hb.ROWWISE_ROWS:
      w, acc, g = hb.rowwise_case(rows, d)
      for aligned in (True, False):
        vec, reread = hb.rowwise_path(d, aligned)
        seen.add((vec, reread))
        label = f"rowwise dense mode {mode} d {d} rows {rows} VEC {vec} REREAD {reread}"
        ref = rw.update(w, acc, g, hp, np.float32, sum_sq=hb.sum_squares_kernel_order(g, vec))
        zero = (g == 0).all(axis=1)
        assert np.array_equal(hb.bits(ref["w"][zero]), hb.bits(w[zero])) and zero.sum() == rows // 5
        wb, ab, gb = _rowwise_dense(w, acc, g, mode, aligned)
        _same(ab[0], _guarded_want(ref["acc"], ab[2]), label + " accumulator")
        _same(wb[0], _guarded_want(ref["w"], wb[2]), label + " table")
        _same(gb[0], _guarded_want(g, gb[2]), label + " gradient")
  assert seen == {(4, False), (4, True), (1, False), (1, True)}


def test_rowwise_dense_kernel_past_the_grid_cap():
  """65 600 rows of d = 256 on the float4 path: 16 400 blocks of lane groups, 16 more than the grid's cap, so the first
  blocks take a second grid-stride iteration.  Compared on the device."""
  rows, d, mode = 65_600, 256, 1
  assert -(-(rows * 64) // 256) > hb.ROWWISE_GRID_CAP
  w, acc, g = hb.rowwise_case(rows, d)
  ref = rw.update(w, acc, g, _rowwise_hyper(mode), np.float32, sum_sq=hb.sum_squares_kernel_order(g, 4))
  wb, ab, gb = _rowwise_dense(w, acc, g, mode, True)
  for buf, want, key in ((wb, ref["w"], "table"), (ab, ref["acc"], "accumulator"), (gb, g, "gradient")):
    want_t = _dev(_guarded_want(want, buf[2]))
    assert torch.equal(buf[0].view(torch.int32), want_t.view(torch.int32)), key
  second = slice(hb.ROWWISE_GRID_CAP * 256 // 64, rows)             # the rows of the second grid-stride iteration
  assert np.array_equal((ref["w"][second] != w[second]).any(axis=1), (g[second] != 0).any(axis=1))
  assert (g[second] != 0).any(axis=1).sum() == 64 - 13


@pytest.mark.parametrize("route", ["rowscan", "sorted"])
@pytest.mark.parametrize("mode", [1, 2])
def test_rowwise_sparse_kernels_in_their_orders(mode, route):
  """``rowwise_adagrad_sorted_kernel<VEC, REREAD>`` (every width of the dense test, vocab 1000) and
  ``rowwise_adagrad_rowscan_kernel<int32 / int64>`` (d <= 256, vocab 37) on the hand-built ids: touched rows and their
  accumulators bit for bit the restatement on the route's summed gradient with the route's sum of squares; untouched rows
  and the row whose summed gradient is zero keep their bits."""
  lib = _lib()
  L = lib.load()
  hp = _rowwise_hyper(mode)
  rowscan = 1 if route == "rowscan" else 0
  vocab = hb.ROWSCAN_VOCAB if rowscan else hb.SORTED_VOCAB
  for d in hb.ROWWISE_DIMS:
    if rowscan and d > 256:
      continue
    rng = np.random.default_rng(100 + d)
    table = hb.rule_weights(rng, (vocab, d))
    acc = hb.rowwise_accumulators(rng, vocab)
    for id_dtype in (np.int32, np.int64):
      label = f"rowwise {route} mode {mode} d {d} {np.dtype(id_dtype).name}"
      case = hb.sparse_ids(vocab, id_dtype)
      ids, rows = case["ids"], hb.sparse_rows(case, d)
      uniq, g = rs.sum_duplicates(ids, rows, vocab, None if rowscan else rs.piece_length(d))
      sum_sq = hb.sum_squares_rowscan_order(g) if rowscan else hb.sum_squares_kernel_order(g, hb.rowwise_path(d, True)[0])
      ref = rw.update(table[uniq], acc[uniq], g, hp, np.float32, sum_sq=sum_sq)
      want_t, want_a = table.copy(), acc.copy()
      want_t[uniq], want_a[uniq] = ref["w"], ref["acc"]
      z = case["zero_pair"]
      assert np.array_equal(hb.bits(want_t[z]), hb.bits(table[z])) and hb.bits(want_a[z]) == hb.bits(acc[z])
      tb, ab = _guarded(table), _guarded(acc)
      ids_t, rows_t = _dev(ids), _dev(rows)
      nbytes = L.tfrs_table_update_workspace_bytes(ids.size, rowscan)
      ws = _workspace(nbytes)
      lib.check(L.tfrs_rowwise_adagrad_sparse(
          lib.ptr(rows_t), lib.ptr(ids_t), 1 if id_dtype == np.int64 else 0, ids.size, d, vocab, lib.ptr(tb[1]),
          lib.ptr(ab[1]), hp["learning_rate"], None, hp["epsilon"], mode, rowscan, lib.ptr(ws), nbytes,
          lib.current_stream()))
      _same(ab[0], _guarded_want(want_a, ab[2]), label + " accumulator")
      _same(tb[0], _guarded_want(want_t, tb[2]), label + " table")


# ---- e. one update, three kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hb.RULE_NAMES)
def test_dense_sorted_and_row_scan_give_the_same_bits(name):
  """Every row of a 37-row table exactly once (no duplicate sum): the dense kernel on the table as one tensor, the sorted
  route and the row scan give the bits of the restatement, hence of one another; d = 8 (float4) and d = 3 (scalar)."""
  lib = _lib()
  L = lib.load()
  kind, hp = hb.rule_hyper(name)
  hyper = (ctypes.c_float * 8)(*hb.rule_hyper_floats(kind, hp))
  vocab = hb.ROWSCAN_VOCAB
  for d in (8, 3):
    rng = np.random.default_rng(500 + d)
    table = hb.rule_weights(rng, (vocab, d))
    slots, t0 = hb.rule_start(name, rng, table)
    alpha = hb.rule_alpha(name, t0)
    ids = hb.unique_ids(vocab, np.int64)
    rows = hb.rule_gradients(rng, (vocab, d))
    dense_g = np.zeros((vocab, d), np.float32)
    dense_g[ids] = rows
    ref = rs.update(kind, table, slots, dense_g, hp, np.float32, alpha=alpha)
    results = {}
    for route in ("rowscan", "sorted"):
      tb, sb = _sparse_rule_call(name, route, d, np.int64, ids, rows, vocab, table, slots, alpha)
      results[route] = [tb[1].cpu().numpy()] + [s[1].cpu().numpy() for s in sb]
    sizes = (vocab * d,)
    p = Packed(sizes, False, [table.reshape(-1)])
    sl = [Packed(sizes, False, [s.reshape(-1)]) for s in slots]
    gp = Packed(sizes, False, [dense_g.reshape(-1)])
    alpha_t = _alpha_dev(alpha)
    lib.check(L.tfrs_table_update_dense_multi(
        hb.RULE_INDEX[kind], hyper, lib.ptr(alpha_t), 1, p.ptrs, sl[0].ptrs if sl else None, sl[1].ptrs if sl else None,
        gp.ptrs, _sizes_arg(sizes), lib.current_stream()))
    o = p.offsets[0]
    results["dense"] = [x.dev[o:o + vocab * d].view(vocab, d).cpu().numpy() for x in [p] + sl]
    want = [ref["w"]] + list(ref["slots"])
    for route, got in results.items():
      for key, x, y in zip(("w",) + rs.SLOTS[kind], got, want):
        assert np.array_equal(hb.bits(x), hb.bits(y)), f"{name} d {d} {route} {key}"
