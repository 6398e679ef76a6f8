"""The embedding kernels (csrc/embedding.hip, csrc/sparse_update.hip) on hand-built id lists (tests/embedding_handbuilt.py, proved on the host by
tests/test_embedding_handbuilt_host.py) at the edges of their layouts that random ids do not reach.

  a. gather_kernel: the tail loop behind the 4-way unrolled one, per_row = 3 and 65, VEC = 1 at d % 4 != 0 and at a
     misaligned table, invalid ids as zero rows with the error flag, and one launch past the grid's cap (both loops in
     one thread, the second grid-stride iteration).
  b. segment_reduce_kernel / segment_reduce_bwd_kernel: bags of 0, 1, 7, 8, 9, 16, 17 and 40 entries (a partly clamped
     round, full rounds, a second round, a last bag whose clamp lands on the final id), int32 and int64 ids / splits,
     VEC = 4 and VEC = 1 (d % 4 != 0, a misaligned gradient), all combiners, exact and arbitrary weights.
  c. rowscan_sum: lists of 1 .. 8193 ids (a partial chunk, exactly one, a chunk and one id, three chunks),
     an id that straddles the chunk boundary, a hit list that has to flush, NS = 1, 2 and 4 at both ends, vocab % 4 != 0
     (dead waves at the barriers); scatter_rowscan_multi_kernel on ten unlike tables (the ninth opens a second launch).
  d. sort_id_positions: one, two and three passes of 8, 9 and 10 bits, each at both ends of its vocabulary range, a single
     key, partial tiles, the two-level scan.
  e. scatter_add_u32_kernel with scatter_add_pieces_kernel, table_update_sorted_kernel and scatter_add_kernel on runs
     placed against the piece cuts, at d < piece and d == piece, VEC = 4 and VEC = 1.

Sums are compared bit for bit with the restatements of the order each route sums in
(``clippy_restatement.sum_duplicates``, ``table_optimizers_restatement.sum_duplicates(..., piece)``).  Every buffer a
kernel writes is a slice of a larger one filled with a sentinel that must survive.  Left to the large tests
(tests/test_baseline_configs_gpu.py): the 4 x 8 plan of the sort (vocab >= 2^30) and the non-temporal variants of the
sorted scatter (tables above 1 GiB)."""

import ctypes

import numpy as np
import pytest

from oracle import embedding as o_emb
from tests import clippy_restatement as crs
from tests import embedding_handbuilt as hb
from tests import table_optimizers_restatement as rs
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4                  # rows of sentinel before and after every buffer a kernel writes
SENTINEL = -7.25e8
U = 2.0 ** -24


def _emb():
  from recommenders_amd.layers import embedding as emb
  return emb


def _lib():
  from recommenders_amd import _lib
  return _lib


def _t(a):
  a = np.ascontiguousarray(a)
  return torch.as_tensor(a if a.flags.writeable else a.copy()).cuda()      # (the shared references are read-only)


def _np(x):
  return x.detach().cpu().numpy()


def _bits(x):
  return hb.bits(_np(x))


class Guarded:
  """``view``: a contiguous [rows, d] float32 slice of a flat buffer with GUARD sentinel rows on either side, filled with
  ``fill`` (16-byte aligned whenever a [rows, d] allocation of its own would be)."""

  def __init__(self, rows, d, fill):
    self.d = d
    self.back = torch.full(((rows + 2 * GUARD) * d,), SENTINEL, dtype=torch.float32, device="cuda")
    self.view = self.back[GUARD * d:(GUARD + rows) * d].view(rows, d)
    if fill is not None:
      self.view.fill_(fill)
    assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

  def assert_guards(self, what=""):
    g = GUARD * self.d
    assert bool((self.back[:g] == SENTINEL).all()) and bool((self.back[self.back.numel() - g:] == SENTINEL).all()), \
        f"{what}: a write outside the buffer"


def _misaligned(a):
  """``a`` on the device as a contiguous view that starts one float into a flat buffer."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  flat = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
  flat[1:] = _t(a).reshape(-1)
  view = flat[1:].view(a.shape)
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  return view


def _dense(vocab, d, uniq, g):
  out = np.zeros((vocab, d), np.float32)
  out[uniq] = g
  return out


# ---- a. gather ----------------------------------------------------------------------------------------------------------
def _gather(table_t, ids_t):
  """tfrs_embedding_gather_fwd into a guarded buffer: (Guarded, error flag)."""
  lib = _lib()
  n, (vocab, d) = ids_t.numel(), table_t.shape
  out = Guarded(n, d, None)
  err = torch.zeros((1,), dtype=torch.int32, device="cuda")
  lib.check(lib.load().tfrs_embedding_gather_fwd(lib.ptr(table_t), vocab, d, lib.ptr(ids_t),
                                                 1 if ids_t.dtype == torch.int64 else 0, n, lib.ptr(out.view),
                                                 lib.ptr(err), lib.current_stream()))
  out.assert_guards("gather")
  return out, int(err.item())


def _check_gather(table_t, table, ids, label):
  emb = _emb()
  vocab = table.shape[0]
  ids_t = _t(ids)
  wide = ids.astype(np.int64)
  ok = (wide >= 0) & (wide < vocab)
  want = np.zeros((ids.size, table.shape[1]), np.float32)
  want[ok] = table[wide[ok]]
  out, flag = _gather(table_t, ids_t)
  assert np.array_equal(_bits(out.view), hb.bits(want)), label
  assert flag == (0 if ok.all() else 1), label
  got = emb.gather_rows(table_t, ids_t)                      # without validate: no exception, the same rows
  assert np.array_equal(_bits(got), hb.bits(want)), label
  if ok.all():
    assert np.array_equal(_bits(emb.gather_rows(table_t, ids_t, validate=True)), hb.bits(want)), label
  else:
    with pytest.raises(IndexError):
      emb.gather_rows(table_t, ids_t, validate=True)


GATHER_SHAPES = [(1, 4), (3, 4), (1027, 12), (1027, 7), (1025, 260), (4099, 5)]


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n,d", GATHER_SHAPES)
def test_gather_at_tail_and_width_edges(n, d, id_dtype):
  """n * per_row is no multiple of 1024 (the tail loop runs; at (1027, 12) and (4099, 5) some threads of the launch take
  the unrolled loop and others the tail), per_row = 3 and 65, VEC = 1 at d = 7 and 5; then the same with 1 % invalid ids
  (at least one) of every kind."""
  vocab = 37
  rng = np.random.default_rng(100 * n + d)
  table = hb.gradient_rows(rng, vocab, d)
  table_t = _t(table)
  ids = rng.integers(0, vocab, size=n).astype(id_dtype)
  ids[-1] = vocab - 1
  _check_gather(table_t, table, ids, "valid")
  bad = ids.copy()
  inv = hb.invalid_ids(vocab, id_dtype)
  for k, pos in enumerate(np.linspace(0, n - 1, num=max(1, n // 100)).astype(np.int64)):
    bad[pos] = inv[k % len(inv)]
  _check_gather(table_t, table, bad, "invalid")


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
def test_gather_from_a_misaligned_table(id_dtype):
  """d % 4 == 0 but the table starts 4 bytes off a 16-byte boundary: the VEC = 1 kernel."""
  vocab, d, n = 37, 8, 1027
  rng = np.random.default_rng(8)
  table = hb.gradient_rows(rng, vocab, d)
  table_t = _misaligned(table)
  ids = rng.integers(0, vocab, size=n).astype(id_dtype)
  _check_gather(table_t, table, ids, "valid")
  ids[::101] = -1
  _check_gather(table_t, table, ids, "invalid")


def test_gather_beyond_one_sweep_of_the_grid():
  """d = 1, n = 2^24 + 1029: more elements than 16384 workgroups x 256 threads x 4, so every thread finishes the unrolled
  loop once and 1029 of them go on into the tail loop, a grid stride further.  Compared on the device."""
  vocab, n = 1000, 2 ** 24 + 1029
  assert n > 16384 * 256 * 4
  rng = np.random.default_rng(24)
  table_t = _t(hb.gradient_rows(rng, vocab, 1))
  ids_t = _t(rng.integers(0, vocab, size=n, dtype=np.int32))
  out, flag = _gather(table_t, ids_t)
  assert flag == 0
  want = table_t[ids_t.long()]
  assert torch.equal(out.view.view(torch.int32), want.view(torch.int32))


# ---- b. combiner --------------------------------------------------------------------------------------------------------
COMBINERS = {"sum": 0, "mean": 1, "sqrtn": 2}


def _segment_fwd(table_t, ids_t, splits_t, w_t, comb):
  lib = _lib()
  assert ids_t.dtype == splits_t.dtype
  nrows, (vocab, d) = splits_t.numel() - 1, table_t.shape
  out = Guarded(nrows, d, None)
  err = torch.zeros((1,), dtype=torch.int32, device="cuda")
  lib.check(lib.load().tfrs_embedding_segment_reduce_fwd(
      lib.ptr(table_t), vocab, d, lib.ptr(ids_t), lib.ptr(splits_t), 1 if ids_t.dtype == torch.int64 else 0,
      lib.ptr(w_t), nrows, COMBINERS[comb], lib.ptr(out.view), lib.ptr(err), lib.current_stream()))
  out.assert_guards("segment_reduce_fwd")
  return out, int(err.item())


def _segment_bwd(grad_t, splits_t, w_t, comb, nnz):
  lib = _lib()
  nrows, d = grad_t.shape
  rows = Guarded(nnz + 1, d, SENTINEL)      # (one spare row: a list without entries still needs a pointer)
  lib.check(lib.load().tfrs_embedding_segment_reduce_bwd(
      lib.ptr(grad_t), d, lib.ptr(splits_t), 1 if splits_t.dtype == torch.int64 else 0, lib.ptr(w_t), nrows,
      COMBINERS[comb], lib.ptr(rows.view), lib.current_stream()))
  rows.assert_guards("segment_reduce_bwd")
  assert bool((rows.view[nnz:] == SENTINEL).all()), "segment_reduce_bwd: a write behind the last entry"
  rows.view = rows.view[:nnz]
  return rows


def _combiner_reference(table, case, w, comb):
  """float64 combiner output and, per entry, sum_j |w_j e_j| / den and the bag length."""
  ids, splits = case["ids"], case["row_splits"]
  nrows, d = splits.size - 1, table.shape[1]
  ref, yard = np.zeros((nrows, d)), np.zeros((nrows, d))
  w64 = np.ones(ids.size) if w is None else w.astype(np.float64)
  for b in range(nrows):
    lo, hi = int(splits[b]), int(splits[b + 1])
    if hi == lo:
      continue
    terms = w64[lo:hi, None] * table[ids[lo:hi]].astype(np.float64)
    den = {"sum": 1.0, "mean": w64[lo:hi].sum(), "sqrtn": np.sqrt((w64[lo:hi] ** 2).sum())}[comb]
    ref[b] = terms.sum(axis=0) / den
    yard[b] = np.abs(terms).sum(axis=0) / den
  return ref, yard, case["lengths"].astype(np.float64)[:, None]


@pytest.mark.parametrize("d", hb.COMBINER_DIMS)
def test_combiner_on_hand_built_bags(d):
  """Forward through ``embedding_lookup_sparse`` (int64) and through the C entry with int32 and int64 ids and splits,
  backward through the C entry with both split types, on the three bag lists.  ``sum`` without weights or with
  power-of-two weights: the oracle bit for bit (every product is exact, so a contracted multiply-add rounds as the
  separate operations do).  Everything else against float64 under (L + 3) 2^-24 sum_j |w_j e_j| / den: one rounding per
  term, one for the denominator, one for the division.  Backward rows within 2^-22 |ref| of the oracle (division and
  product, each at most one ulp)."""
  emb = _emb()
  vocab = 50
  table = hb.gradient_rows(np.random.default_rng(d), vocab, d)
  table_t = _t(table)
  for kind in ("empty_last", "full_last", "all_empty"):
    case = hb.bag_case(kind, vocab)
    ids, splits = case["ids"], case["row_splits"]
    nrows, nnz = splits.size - 1, ids.size
    i64 = (_t(ids), _t(splits))
    i32 = (_t(ids.astype(np.int32)), _t(splits.astype(np.int32)))
    grad = hb.gradient_rows(np.random.default_rng(1000 + d), nrows, d)
    grad_t = _t(grad)
    for wkind in ("none", "pow2", "any"):
      w = None if wkind == "none" else hb.bag_weights(case, wkind)
      w_t = None if w is None else _t(w)
      for comb in COMBINERS:
        label = f"{kind} d {d} {wkind} {comb}"
        out64, flag = _segment_fwd(table_t, i64[0], i64[1], w_t, comb)
        out32, flag32 = _segment_fwd(table_t, i32[0], i32[1], w_t, comb)
        assert flag == 0 and flag32 == 0, label
        got = _np(out64.view)
        assert np.array_equal(hb.bits(got), _bits(out32.view)), label
        wrapped = emb.embedding_lookup_sparse(table_t, i64[0], i64[1], w_t, combiner=comb, validate=True)
        assert np.array_equal(hb.bits(got), _bits(wrapped)), label
        assert (hb.bits(got[case["lengths"] == 0]) == 0).all(), label          # empty bags: +0
        if comb == "sum" and wkind != "any":
          assert np.array_equal(hb.bits(got), hb.bits(o_emb.lookup_sparse(table, ids, splits, w, comb))), label
        ref, yard, length = _combiner_reference(table, case, w, comb)
        float_gate(f"embedding_layout.segment_fwd.{comb}.{wkind}", got, ref, (length + 3.0) * yard, U)
        # backward
        want = o_emb.lookup_sparse_grad_rows(grad, splits, w, comb)
        rows64 = _segment_bwd(grad_t, i64[1], w_t, comb, nnz)
        rows32 = _segment_bwd(grad_t, i32[1], w_t, comb, nnz)
        assert np.array_equal(_bits(rows64.view), _bits(rows32.view)), label
        float_gate(f"embedding_layout.segment_bwd.{comb}.{wkind}", _np(rows64.view), want, np.abs(want), 4 * U)
        if d == 12:       # d % 4 == 0 from a misaligned gradient: VEC = 1, the same bits
          rows_m = _segment_bwd(_misaligned(grad), i64[1], w_t, comb, nnz)
          assert np.array_equal(_bits(rows64.view), _bits(rows_m.view)), label


@pytest.mark.parametrize("d", [4, 7])
def test_combiner_ignores_an_invalid_id_inside_a_bag(d):
  """-1 and vocab inside the 40-entry bag and as the last id of the list: the sum is the oracle's without those entries
  (bit for bit), the error flag is set and ``validate=True`` raises."""
  emb = _emb()
  vocab = 50
  table = hb.gradient_rows(np.random.default_rng(d), vocab, d)
  case = hb.bag_case("full_last", vocab)
  ids, splits = case["ids"].copy(), case["row_splits"]
  bad = np.array([3, 17, ids.size - 1])
  ids[bad] = [-1, vocab, vocab]
  for wkind in ("none", "pow2"):
    w = np.ones(ids.size, np.float32) if wkind == "none" else hb.bag_weights(case, wkind)
    w_ref = w.copy()
    w_ref[bad] = 0.0                                          # acc + 0 * e is acc: the entry contributes nothing
    want = o_emb.lookup_sparse(table, np.where((ids >= 0) & (ids < vocab), ids, 0), splits, w_ref, "sum")
    w_t = None if wkind == "none" else _t(w)
    for cast in (np.int32, np.int64):
      out, flag = _segment_fwd(_t(table), _t(ids.astype(cast)), _t(splits.astype(cast)), w_t, "sum")
      assert flag == 1
      assert np.array_equal(_bits(out.view), hb.bits(want)), (wkind, cast)
    with pytest.raises(IndexError):
      emb.embedding_lookup_sparse(_t(table), _t(ids), _t(splits), w_t, combiner="sum", validate=True)
    got = emb.embedding_lookup_sparse(_t(table), _t(ids), _t(splits), w_t, combiner="sum")
    assert np.array_equal(_bits(got), hb.bits(want))


# ---- c. row scan --------------------------------------------------------------------------------------------------------
ROWSCAN_DIMS = hb.ROWSCAN_DIMS
_CHUNK_REFERENCE = {}


def _chunk_reference(n, vocab):
  """(rows [n, 256], uniq, sums [len(uniq), 256]) of the chunk case, computed once and read-only: the columns of a sum
  do not depend on one another, so width d takes the first d of them.  (The int32 and the int64 list hold their valid
  ids at the same positions.)"""
  if (n, vocab) not in _CHUNK_REFERENCE:
    rows = hb.gradient_rows(np.random.default_rng(31 * n + vocab), n, 256)
    uniq, g = crs.sum_duplicates(hb.chunk_case(n, vocab)["ids"], rows, vocab)
    for a in (rows, uniq, g):
      a.setflags(write=False)
    _CHUNK_REFERENCE[(n, vocab)] = (rows, uniq, g)
  return _CHUNK_REFERENCE[(n, vocab)]


def _rowscan(rows_t, ids_t, vocab, dst, accum=None, lr=0.0, eps=0.0, mode=0):
  lib = _lib()
  n, d = ids_t.numel(), dst.shape[1]
  assert d <= 256 and dst.shape[0] == vocab and (n == 0 or tuple(rows_t.shape) == (n, d))
  lib.check(lib.load().tfrs_embedding_scatter_add_rowscan(
      lib.ptr(rows_t), lib.ptr(ids_t), 1 if ids_t.dtype == torch.int64 else 0, n, d, vocab, lib.ptr(dst),
      lib.ptr(accum), lr, eps, mode, lib.current_stream()))


def _check_adagrad(table, acc, uniq, g, vocab, legacy, label, lr=0.5, eps=1e-7):
  """A fused Adagrad step from table 0 / accumulator 0.1 (``table``, ``acc``: Guarded, after the step) against the
  formula on the summed gradient ``g``: the tolerances of test_embedding_layer_autograd_and_adagrad; untouched rows keep
  their bits; the sentinels survive."""
  table.assert_guards(label)
  acc.assert_guards(label)
  untouched = np.ones(vocab, bool)
  untouched[uniq] = False
  got_w, got_a = _np(table.view), _np(acc.view)
  assert (hb.bits(got_w[untouched]) == 0).all(), label
  assert (hb.bits(got_a[untouched]) == hb.bits(np.float32(0.1))).all(), label
  g64 = g.astype(np.float64)
  a_ref = np.float64(np.float32(0.1)) + g64 * g64
  den = np.sqrt(a_ref) + eps if legacy else np.sqrt(a_ref + eps)
  np.testing.assert_allclose(got_a[uniq], a_ref, rtol=1e-6, err_msg=label)
  np.testing.assert_allclose(got_w[uniq], -lr * g64 / den, rtol=1e-5, atol=1e-7, err_msg=label)


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("d", ROWSCAN_DIMS)
def test_row_scan_across_chunks_and_flushes(d, id_dtype):
  emb = _emb()
  for n in hb.CHUNK_NS:
    for vocab in hb.CHUNK_VOCABS:
      label = f"n {n} vocab {vocab} d {d}"
      case = hb.chunk_case(n, vocab, id_dtype)
      rows256, uniq, g256 = _chunk_reference(n, vocab)
      rows_t, ids_t = _t(rows256[:, :d]), _t(case["ids"])
      g = g256[:, :d]
      assert emb._use_rowscan(vocab, n, d)
      want = _dense(vocab, d, uniq, g)
      out = Guarded(vocab, d, None)                    # dense mode writes every row: untouched ones as +0
      _rowscan(rows_t, ids_t, vocab, out.view)
      out.assert_guards(label)
      assert np.array_equal(_bits(out.view), hb.bits(want)), label
      assert np.array_equal(_bits(emb.scatter_add_rows(rows_t, ids_t, vocab)), hb.bits(want)), label
      for legacy in (False, True):
        table, acc = Guarded(vocab, d, 0.0), Guarded(vocab, d, 0.1)
        emb.adagrad_sparse_update_(table.view, acc.view, rows_t, ids_t, lr=0.5, legacy=legacy)
        _check_adagrad(table, acc, uniq, g, vocab, legacy, label)


MULTI_TABLES = [  # (vocab, d, id dtype, n): the ninth opens a second launch
    (7, 1, np.int64, 4097), (1, 63, np.int32, 4095), (5, 64, np.int64, 8193), (8, 65, np.int32, 4096),
    (2, 128, np.int64, 1), (7, 129, np.int32, 0), (5, 256, np.int64, 4097), (8, 7, np.int32, 8193),
    (2, 200, np.int64, 4095), (7, 32, np.int32, 4097)]


@pytest.mark.parametrize("legacy", [False, True])
def test_multi_table_row_scan_equals_the_single_calls(legacy):
  """Ten tables of different (vocab, d, id dtype) in ``adagrad_sparse_update_multi_`` -- one without ids, one of a single
  row, one at d = 256; eight go into the first launch and two into a second -- against ten single calls, bit for bit,
  tables, accumulators and sentinels alike."""
  emb = _emb()
  assert len(MULTI_TABLES) == 10
  multi, single, updates = [], [], []
  for vocab, d, id_dtype, n in MULTI_TABLES:
    assert emb._use_rowscan(vocab, n, d)
    if n:
      ids = hb.chunk_case(n, vocab, id_dtype)["ids"]
      rows = _chunk_reference(n, vocab)[0][:, :d]
    else:
      ids, rows = np.zeros((0,), id_dtype), np.zeros((0, d), np.float32)
    rows_t, ids_t = _t(rows), _t(ids)
    start = hb.gradient_rows(np.random.default_rng(vocab + d), vocab, d, negative_zeros=False)
    pair = []
    for dest in (multi, single):
      table, acc = Guarded(vocab, d, None), Guarded(vocab, d, 0.1)
      table.view.copy_(_t(start))
      dest.append((table, acc))
      pair.append((table.view, acc.view, rows_t, ids_t))
    updates.append(pair[0])
    emb.adagrad_sparse_update_(*pair[1], lr=0.5, legacy=legacy)
  emb.adagrad_sparse_update_multi_(updates, lr=0.5, legacy=legacy)
  changed = 0
  for k, ((mt, ma), (st, sa)) in enumerate(zip(multi, single)):
    assert torch.equal(mt.back.view(torch.int32), st.back.view(torch.int32)), k
    assert torch.equal(ma.back.view(torch.int32), sa.back.view(torch.int32)), k
    mt.assert_guards(f"table {k}")
    ma.assert_guards(f"accumulator {k}")
    changed += int(bool((ma.view != 0.1).any()))
  assert changed == 9                                   # every table but the one without ids was updated


# ---- d. the sort's plans ------------------------------------------------------------------------------------------------
@pytest.fixture
def sorted_route(monkeypatch):
  monkeypatch.setattr(_emb(), "_ROWSCAN_MAX_WORK", 0)


def _sorted_dense(rows_t, ids_t, vocab, view):
  """The sorted route's dense gradient into ``view`` (zeroed first, as ``scatter_add_rows`` does)."""
  view.zero_()
  _emb()._scatter_unsorted(rows_t, ids_t, vocab, view, None, 0.0, 0.0, 0)


@pytest.mark.parametrize("vocab", sorted(hb.SORT_PLANS))
def test_sorted_scatter_at_every_sort_plan(vocab, sorted_route):
  """The plan of ``vocab`` (hb.SORT_PLANS, asserted against the library on the host and here) on lists of 1, 4095, 4097
  and 70001 ids that hold 0, vocab - 1, ids apart in the top digit only and in the bottom digit only, and long runs: the
  touched rows equal the piece-order restatement bit for bit and nothing else of the gradient is non-zero.  Compared on
  the device; nothing dense is built on the host."""
  emb, lib = _emb(), _lib()
  passes, digit_bits = ctypes.c_int(), ctypes.c_int()
  lib.check(lib.load().tfrs_embedding_sort_plan(vocab, ctypes.byref(passes), ctypes.byref(digit_bits)))
  assert (passes.value, digit_bits.value) == hb.SORT_PLANS[vocab]
  d = 1 if vocab == 2 ** 27 else 4
  piece = rs.piece_length(d)
  id_dtype = np.int32 if sorted(hb.SORT_PLANS).index(vocab) % 2 else np.int64
  out = Guarded(vocab, d, None)
  for n in hb.SORT_NS:
    ids, _ = hb.sort_plan_ids(vocab, n, *hb.SORT_PLANS[vocab])
    rows = hb.gradient_rows(np.random.default_rng(n + d), n, d)
    uniq, g = rs.sum_duplicates(ids, rows, vocab, piece)
    assert not emb._use_rowscan(vocab, n, d)
    rows_t, ids_t = _t(rows), _t(ids.astype(id_dtype))
    _sorted_dense(rows_t, ids_t, vocab, out.view)
    out.assert_guards(f"vocab {vocab} n {n}")
    got = out.view[_t(uniq)]
    assert np.array_equal(_bits(got), hb.bits(g)), (vocab, n)
    assert int(torch.count_nonzero(out.view)) == int(np.count_nonzero(g)), (vocab, n)
    if vocab <= 2 ** 19:
      wrapped = emb.scatter_add_rows(rows_t, ids_t, vocab)
      assert torch.equal(wrapped.view(torch.int32), out.view.view(torch.int32)), (vocab, n)


# ---- e. run layouts on the sorted route ---------------------------------------------------------------------------------
RUN_DIMS = hb.RUN_DIMS


def _sgd_table(vocab, d):
  """A zero table inside guard rows as a Parameter that ``optimizers.SGD`` takes slices for."""
  table = Guarded(vocab, d, 0.0)
  p = torch.nn.Parameter(table.view)
  assert p.data_ptr() == table.view.data_ptr()
  p._tfrs_embedding = True
  return table, p


def _run_layout_checks(d, id_dtype, misaligned):
  emb = _emb()
  from recommenders_amd.optimizers import SGD
  piece = rs.piece_length(d)
  for variant in hb.RUN_VARIANTS:
    label = f"{variant} d {d}"
    case = hb.run_layout_case(piece, variant, id_dtype)
    ids, vocab, n = case["ids"], case["vocab"], case["n"]
    rows = hb.run_layout_rows(case, d)
    uniq, g = rs.sum_duplicates(ids, rows, vocab, piece)
    want = _dense(vocab, d, uniq, g)
    rows_t, ids_t = (_misaligned(rows) if misaligned else _t(rows)), _t(ids)
    assert not emb._use_rowscan(vocab, n, d)
    # scatter_add_rows
    out = Guarded(vocab, d, None)
    _sorted_dense(rows_t, ids_t, vocab, out.view)
    out.assert_guards(label)
    assert np.array_equal(_bits(out.view), hb.bits(want)), label
    assert np.array_equal(_bits(emb.scatter_add_rows(rows_t, ids_t, vocab)), hb.bits(want)), label
    # fused Adagrad
    for legacy in (False, True):
      table, acc = Guarded(vocab, d, 0.0), Guarded(vocab, d, 0.1)
      emb.adagrad_sparse_update_(table.view, acc.view, rows_t, ids_t, lr=0.5, legacy=legacy)
      _check_adagrad(table, acc, uniq, g, vocab, legacy, label)
    # SGD at rate one on a zero table: table_update_sorted_kernel on the same list
    table, p = _sgd_table(vocab, d)
    opt = SGD([p], learning_rate=1.0)
    p._tfrs_slices.append((ids_t, rows_t))
    opt.step()
    table.assert_guards(label + " SGD")
    assert np.array_equal(_bits(table.view), hb.bits(np.float32(0) - want)), label     # (0 - (+0) is +0, not -0)
    assert (hb.bits(_np(table.view)[np.setdiff1d(np.arange(vocab), uniq)]) == 0).all(), label
    opt.close()
    # every run shorter than a piece: the row scan sums in the same order
    if variant in ("short", "all_invalid"):
      scan = Guarded(vocab, d, None)
      _rowscan(rows_t, ids_t, vocab, scan.view)
      scan.assert_guards(label + " row scan")
      assert torch.equal(scan.view.view(torch.int32), out.view.view(torch.int32)), label


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("d", RUN_DIMS)
def test_sorted_route_on_runs_at_the_piece_cuts(d, id_dtype, sorted_route):
  """Every variant of the run-layout case at piece_length(d): the dense gradient equals the piece-order restatement bit
  for bit (d = 32, 64, 128: d == piece, where the partial sums use all of the sort's spare key buffer; that buffer is
  inside the library's workspace, so a write behind it is NOT observable here -- only the sums are checked), the fused
  Adagrad takes the same sums, ``SGD(learning_rate=1)`` on a zero table is minus that gradient, and where no run reaches
  a piece the row scan gives the same bits."""
  _run_layout_checks(d, id_dtype, misaligned=False)


def test_sorted_route_from_a_misaligned_gradient(sorted_route):
  """d = 8 from rows that start 4 bytes off a 16-byte boundary: the VEC = 1 scatter and pieces at d % 4 == 0."""
  _run_layout_checks(8, np.int64, misaligned=True)


@pytest.mark.parametrize("d", [8, 7])
def test_scatter_add_bwd_on_presorted_ids(d):
  """``tfrs_embedding_scatter_add_bwd`` (int64 ids sorted by a stable argsort, with their positions; invalid ids mapped
  to -1, which it skips): one sequential chain per run, so the single-chain restatement bit for bit."""
  lib = _lib()
  case = hb.run_layout_case(rs.piece_length(d), "invalid")
  ids, vocab, n = case["ids"].astype(np.int64), case["vocab"], case["n"]
  rows = hb.run_layout_rows(case, d)
  uniq, g = crs.sum_duplicates(ids, rows, vocab)
  clean = np.where((ids >= 0) & (ids < vocab), ids, -1)
  perm = np.argsort(clean, kind="stable").astype(np.int64)
  sorted_ids = clean[perm]
  assert sorted_ids.min() == -1 and sorted_ids.max() == vocab - 1 and perm.min() == 0 and perm.max() == n - 1
  out = Guarded(vocab, d, 0.0)
  rows_t, sorted_t, perm_t = _t(rows), _t(sorted_ids), _t(perm)
  lib.check(lib.load().tfrs_embedding_scatter_add_bwd(lib.ptr(rows_t), lib.ptr(sorted_t), lib.ptr(perm_t), n, d,
                                                      lib.ptr(out.view), None, 0.0, 0.0, 0, lib.current_stream()))
  out.assert_guards("scatter_add_bwd")
  assert np.array_equal(_bits(out.view), hb.bits(_dense(vocab, d, uniq, g)))
