"""The integer kernels in front of the embedding tables on hand-built inputs (tests/ids_handbuilt.py, proved on the
host by tests/test_ids_handbuilt_host.py), through the C entry points, every comparison exact.

  A. ``tfrs_shard_route_ids`` (csrc/shard_route.hip): the scan at per = 1, 2, 9 and 17 (a full chunk of 8 followed by
     a partial one, two full chunks, lanes with nothing behind lanes with several chunks), owner patterns that fill
     whole segments and tiles with one owner, leave owners empty or consist of invalid ids, world 1 .. 64, ranks
     without rows, one row per rank, a table beyond 2^40 rows, the entry checks.
  B. ``tfrs_unified_embedding_fwd`` / ``_multi`` (csrc/hashing.hip): every PER_ROW x id width of both kernels and the
     packed-strings form, 1 .. 3 launches with their ``out_chunk0`` / ``bucket_col0``, total % 64 in {0, 1, 63}, one
     value, the grid-stride pass behind the grid cap, ``buckets`` itself and ``buckets = NULL``, the refusals.
  C. ``tfrs_hash_bucket_strong_ids`` / ``_bytes`` and ``tfrs_fingerprint_bytes`` past their grid cap; ``num_bins`` up to
     2^63 - 1.
  D. ``tfrs_row_hash64`` (csrc/dedup.hip): 1 .. 32 lanes per row, piece counts that are no power of two or exceed the
     lanes, the scalar kernel (d % 4 != 0, a base that is not 16-byte aligned); ``BruteForce(dedup=True)`` on top.

Every buffer a kernel writes lies inside a larger one whose sentinels must survive; the routing workspace is exactly
``tfrs_shard_route_workspace_bytes`` long and filled with 0xFF.  References: the NumPy / Python-int restatements of
tests/ids_handbuilt.py and ``oracle/hashing.py``; never a second run of a kernel."""

import ctypes

import numpy as np
import pytest

from oracle import hashing as o_hash
from oracle import topk as o_topk
from tests import ids_handbuilt as hb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 256                        # sentinel elements before and after every buffer a kernel writes
F_SENT = -(2.0 ** 30)              # float32 outputs (no table cell is negative)
I64_SENT = 0x5A5A5A5A5A5A5A5A      # no bucket, local row, count or 63-bit hash used here has this value
I32_SENT = -0x5A5A5A5B             # positions are >= 0
SENTINELS = {"float32": F_SENT, "int64": I64_SENT, "int32": I32_SENT, "uint8": 0xA5}
WS_FILL = 0xFF


def _L():
  from recommenders_amd import _lib
  return _lib


def _t(a):
  a = np.ascontiguousarray(a)
  return torch.as_tensor(a if a.flags.writeable else a.copy()).cuda()      # (the shared references are read-only)


def _np(x):
  return x.detach().cpu().numpy()


class Guarded:
  """``view``: a contiguous tensor of ``shape`` inside a flat buffer with GUARD sentinels on either side (256-byte
  aligned like an allocation of its own).  The view itself starts as ``fill`` (default: the sentinel too)."""

  def __init__(self, shape, dtype, fill=None):
    self.sentinel = SENTINELS[str(dtype).split(".")[-1]]
    numel = int(np.prod(shape, dtype=np.int64))
    self.back = torch.full((numel + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda")
    self.view = self.back[GUARD:GUARD + numel].view(shape)
    if fill is not None:
      self.view.fill_(fill)
    assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

  def assert_guards(self, what=""):
    assert bool((self.back[:GUARD] == self.sentinel).all()), f"{what}: a write in front of the buffer"
    assert bool((self.back[self.back.numel() - GUARD:] == self.sentinel).all()), f"{what}: a write behind the buffer"

  def assert_untouched(self, what=""):
    assert bool((self.back == self.sentinel).all()), f"{what}: the buffer was written"


def _same_bits(got, want):
  want = _t(want)
  assert got.shape == want.shape and got.dtype == want.dtype
  if got.dtype == torch.float32:
    got, want = got.view(torch.int32), want.view(torch.int32)
  if not torch.equal(got, want):
    bad = torch.nonzero(got != want)
    first = tuple(bad[0].tolist())
    raise AssertionError(f"{bad.shape[0]} of {got.numel()} entries differ; first at {first}: "
                         f"got {got[first].item()}, want {want[first].item()}")


# ================================================================================================ A. shard routing
class _RouteBuffers:
  def __init__(self, n, world, ws_bytes):
    self.send = Guarded((n,), torch.int64)
    self.perm = Guarded((n,), torch.int32)
    self.order = Guarded((n,), torch.int32)
    self.counts = Guarded((world,), torch.int64)
    self.ws = Guarded((ws_bytes,), torch.uint8, fill=WS_FILL)
    self.ws_bytes = ws_bytes

  def all(self):
    return (("send_ids", self.send), ("perm", self.perm), ("order", self.order), ("counts", self.counts),
            ("workspace", self.ws))

  def assert_guards(self):
    for name, buf in self.all():
      buf.assert_guards(name)


def _route_call(ids_t, n, input_dim, rows_per_rank, world, buf, null=None, ws_bytes=None):
  lib = _L()
  p = {"ids": lib.ptr(ids_t), "send_ids": lib.ptr(buf.send.view), "perm": lib.ptr(buf.perm.view),
       "order": lib.ptr(buf.order.view), "counts": lib.ptr(buf.counts.view), "workspace": lib.ptr(buf.ws.view)}
  if null is not None:
    p[null] = lib.ptr(None)
  rc = lib.load().tfrs_shard_route_ids(p["ids"], 1 if ids_t.dtype == torch.int64 else 0, n, input_dim, rows_per_rank,
                                       world, p["send_ids"], p["perm"], p["order"], p["counts"], p["workspace"],
                                       buf.ws_bytes if ws_bytes is None else ws_bytes, lib.current_stream())
  torch.cuda.synchronize()
  return rc


ROUTE_PARAMS = [(name, width) for name in hb.ROUTE_NAMES for width in ("int64", "int32")
                if width == "int64" or name not in hb.ROUTE_WIDE]


@pytest.mark.parametrize("name,width", ROUTE_PARAMS)
def test_shard_route(name, width):
  lib = _L()
  case = hb.route_case(name)
  n, world = case.n, case.world
  ids_t = _t(case.ids.astype(np.int32) if width == "int32" else case.ids)
  assert width == "int64" or np.array_equal(_np(ids_t).astype(np.int64), case.ids)
  ws_bytes = int(lib.load().tfrs_shard_route_workspace_bytes(n, world))
  assert ws_bytes == hb.workspace_bytes(n, world)
  buf = _RouteBuffers(n, world, ws_bytes)
  assert _route_call(ids_t, n, case.input_dim, case.rows_per_rank, world, buf) == lib.TFRS_OK, lib.last_error()
  send, perm, order, counts = case.expected
  assert _np(buf.counts.view).tolist() == counts.tolist()
  _same_bits(buf.send.view, send)
  _same_bits(buf.perm.view, perm)
  _same_bits(buf.order.view, order)
  assert torch.equal(buf.order.view[buf.perm.view.long()].long(), torch.arange(n, device="cuda"))
  buf.assert_guards()


def test_shard_route_entry_checks():
  lib = _L()
  n, dim, rpr, world = 5000, 1000, 125, 8
  ids_t = _t(np.arange(n, dtype=np.int64) % dim)
  ws_bytes = int(lib.load().tfrs_shard_route_workspace_bytes(n, 65))       # enough for every call below
  buf = _RouteBuffers(n, 65, ws_bytes)

  def untouched():
    for name, b in buf.all():
      if name == "workspace":
        assert bool((b.view == WS_FILL).all()) and b.assert_guards(name) is None
      else:
        b.assert_untouched(name)

  assert _route_call(ids_t, n, dim, 16, 65, buf) == lib.TFRS_EINVAL                  # world = 65
  assert _route_call(ids_t, n, dim, 124, world, buf) == lib.TFRS_EINVAL              # 124 x 8 = 992 < 1000 rows
  assert _route_call(ids_t, -1, dim, rpr, world, buf) == lib.TFRS_EINVAL             # n < 0
  for null in ("ids", "send_ids", "perm", "order", "counts", "workspace"):
    assert _route_call(ids_t, n, dim, rpr, world, buf, null=null) == lib.TFRS_EINVAL, null
  need = int(lib.load().tfrs_shard_route_workspace_bytes(n, world))
  assert need == hb.workspace_bytes(n, world)
  assert _route_call(ids_t, n, dim, rpr, world, buf, ws_bytes=need - 1) == lib.TFRS_ENOMEM
  untouched()
  # n = 0 zeroes counts[world] and touches nothing else
  assert _route_call(ids_t, 0, dim, rpr, world, buf) == lib.TFRS_OK
  assert _np(buf.counts.view).tolist() == [0] * world + [I64_SENT] * (65 - world)
  buf.counts.view.fill_(I64_SENT)
  untouched()
  # ... and the same call with exactly the stated workspace goes through
  exact = _RouteBuffers(n, world, need)
  assert _route_call(ids_t, n, dim, rpr, world, exact) == lib.TFRS_OK
  assert _np(exact.counts.view).tolist() == [n // world] * world
  exact.assert_guards()


# ================================================================================================ B. fused lookups
def _device_tables(units, num_bins, d):
  return {t: _t(hb.make_table(t, num_bins, d)) for t in sorted({hb.table_of(u) for u in units})}


def _u64(values):
  return (ctypes.c_uint64 * len(values))(*values)


def _vp(values):
  return (ctypes.c_void_p * len(values))(*values)


def _unified(kind, n, chunks, num_bins, d, keep_buckets=True):
  """One ``tfrs_unified_embedding_fwd`` call on periodic values, checked against ``hb.unified_expected``."""
  lib = _L()
  tabs = _device_tables(range(chunks), num_bins, d)
  ids = blob = offsets = None
  if kind == "bytes":
    blob, offsets = (_t(a) for a in hb.pack_periodic(hb.base_strings(), n))
  else:
    ids = _t(hb.base_ids(kind)[np.arange(n) % hb.PERIOD])
  out = Guarded((n, chunks * d), torch.float32)
  buckets = Guarded((n, chunks), torch.int64)
  salts = [hb.salt_of(c) for c in range(chunks)]
  rc = lib.load().tfrs_unified_embedding_fwd(
      lib.ptr(ids), 1 if kind == "i64" else 0, lib.ptr(blob), lib.ptr(offsets), n, chunks,
      _vp([tabs[hb.table_of(c)].data_ptr() for c in range(chunks)]), _u64([s[0] for s in salts]),
      _u64([s[1] for s in salts]), num_bins, d, lib.ptr(out.view), lib.ptr(buckets.view if keep_buckets else None),
      lib.current_stream())
  torch.cuda.synchronize()
  assert rc == lib.TFRS_OK, lib.last_error()
  want_out, want_buckets = hb.unified_expected(kind, n, chunks, num_bins, d, F_SENT)
  _same_bits(out.view, want_out)
  out.assert_guards("out")
  if keep_buckets:
    _same_bits(buckets.view, want_buckets)
    buckets.assert_guards("buckets")
  else:
    buckets.assert_untouched("buckets")


def _multi(kind, n, units, num_bins, d, keep_buckets=True):
  """One ``tfrs_unified_embedding_fwd_multi`` call, checked against ``hb.multi_expected``."""
  lib = _L()
  feature, chunk, declared = hb.multi_layout(units)
  tabs = _device_tables(range(units), num_bins, d)
  ids = [_t(hb.multi_ids(kind, n, f)) for f in range(len(declared))]
  outs = [Guarded((n, c * d), torch.float32) for c in declared]
  buckets = Guarded((n, units), torch.int64)
  salts = [hb.salt_of(u) for u in range(units)]
  i32 = ctypes.c_int32 * units
  rc = lib.load().tfrs_unified_embedding_fwd_multi(
      units, _vp([ids[f].data_ptr() for f in feature]), 1 if kind == "i64" else 0, n,
      _vp([tabs[hb.table_of(u)].data_ptr() for u in range(units)]), _u64([s[0] for s in salts]),
      _u64([s[1] for s in salts]), num_bins, d, _vp([outs[f].view.data_ptr() for f in feature]),
      i32(*[declared[f] for f in feature]), i32(*chunk), lib.ptr(buckets.view if keep_buckets else None),
      lib.current_stream())
  torch.cuda.synchronize()
  assert rc == lib.TFRS_OK, lib.last_error()
  want_outs, want_buckets = hb.multi_expected(kind, n, units, num_bins, d, F_SENT)
  for f, (got, want) in enumerate(zip(outs, want_outs)):
    _same_bits(got.view, want)               # (the column blocks of a cut last feature keep their sentinel)
    got.assert_guards(f"out of feature {f}")
  if keep_buckets:
    _same_bits(buckets.view, want_buckets)
    buckets.assert_guards("buckets")
  else:
    buckets.assert_untouched("buckets")


@pytest.mark.parametrize("kind", ["i32", "i64", "bytes"])
@pytest.mark.parametrize("d", hb.DIMS)
def test_unified_every_per_row(d, kind):
  _unified(kind, 300, 3, 37, d)              # 900 lookups: four blocks, a last wave of 4 lanes


@pytest.mark.parametrize("kind", ["i32", "i64"])
@pytest.mark.parametrize("d", hb.DIMS)
def test_unified_multi_every_per_row(d, kind):
  _multi(kind, 300, 5, 37, d)                # features of 1, 3 and (cut) 2 chunks


@pytest.mark.parametrize("num_bins", [1, 256])
@pytest.mark.parametrize("d", [4, 16, 256])
def test_unified_num_bins_edges(d, num_bins):
  _unified("i64", 130, 4, num_bins, d)
  _multi("i32", 130, 4, num_bins, d)


@pytest.mark.parametrize("chunks,n", [(1, 1), (1, 64), (1, 65), (1, 127), (3, 21), (3, 43), (3, 64), (16, 1), (16, 300),
                                      (17, 300), (33, 300), (33, 1), (17, 67)])
def test_unified_launches_and_wave_tails(chunks, n):
  """n_chunks 1, 16, 17, 33: one, two and three launches (out_chunk0 = 0, 16, 32); totals with a last wave of 64, 1
  and 63 lanes; a single value."""
  _unified("i64", n, chunks, 37, 16)


@pytest.mark.parametrize("units,n", [(1, 1), (1, 64), (1, 65), (1, 127), (64, 67), (65, 67), (129, 67), (129, 1)])
def test_unified_multi_units_and_wave_tails(units, n):
  """n_units 1, 64, 65, 129: one, two and three launches (bucket_col0 = 0, 64, 128), features of 1, 3, 2 and 5 chunks
  of which two straddle a launch boundary."""
  _multi("i64", n, units, 37, 16)


def test_unified_past_the_grid_cap():
  _unified("i64", hb.N_LOOKUP_PAST_CAP, 16, 256, 4)


def test_unified_multi_past_the_grid_cap():
  _multi("i32", hb.N_LOOKUP_PAST_CAP, 16, 256, 4)


@pytest.mark.parametrize("d", [4, 64])
def test_unified_without_buckets(d):
  _unified("i64", 300, 17, 37, d, keep_buckets=False)
  _unified("bytes", 300, 2, 37, d, keep_buckets=False)
  _multi("i64", 300, 65, 37, d, keep_buckets=False)


def _misaligned_f32(shape):
  flat = torch.zeros((int(np.prod(shape)) + 1,), dtype=torch.float32, device="cuda")
  view = flat[1:].view(shape)
  assert view.data_ptr() % 16 == 4
  return view


def test_unified_refusals():
  lib = _L()
  fn, fn_multi = lib.load().tfrs_unified_embedding_fwd, lib.load().tfrs_unified_embedding_fwd_multi
  n, bins = 40, 37
  ids = _t(hb.base_ids("i64")[:n])
  out = Guarded((n, 2 * 512), torch.float32)
  buckets = Guarded((n, 2), torch.int64)
  table = _t(np.zeros((bins, 512), np.float32))
  salts = _u64([1, 2])
  i32x2 = ctypes.c_int32 * 2

  def single(d, out_t=None, tables=None, n_values=n):
    rc = fn(lib.ptr(ids), 1, lib.ptr(None), lib.ptr(None), n_values, 2,
            _vp(tables or [table.data_ptr()] * 2), salts, salts, bins, d,
            lib.ptr(out.view if out_t is None else out_t), lib.ptr(buckets.view), lib.current_stream())
    torch.cuda.synchronize()
    return rc

  def multi(d, out_t=None, tables=None, n_values=n, chunk_index=(0, 1), feature_chunks=(2, 2)):
    o = (out.view if out_t is None else out_t).data_ptr()
    rc = fn_multi(2, _vp([ids.data_ptr()] * 2), 1, n_values, _vp(tables or [table.data_ptr()] * 2), salts, salts,
                  bins, d, _vp([o, o]), i32x2(*feature_chunks), i32x2(*chunk_index), lib.ptr(buckets.view),
                  lib.current_stream())
    torch.cuda.synchronize()
    return rc

  for call in (single, multi):
    assert call(12) == lib.TFRS_ENOTIMPL and call(512) == lib.TFRS_ENOTIMPL
    assert call(4, out_t=_misaligned_f32((n, 8))) == lib.TFRS_EINVAL
    assert call(4, tables=[table.data_ptr(), _misaligned_f32((bins, 4)).data_ptr()]) == lib.TFRS_EINVAL
    assert call(4, n_values=0) == lib.TFRS_OK
  assert multi(4, chunk_index=(0, 2)) == lib.TFRS_EINVAL                   # chunk_index >= feature_chunks
  assert multi(4, chunk_index=(0, 1), feature_chunks=(2, 1)) == lib.TFRS_EINVAL
  assert multi(4, chunk_index=(0, -1)) == lib.TFRS_EINVAL
  out.assert_untouched("out")
  buckets.assert_untouched("buckets")


# ================================================================================================ C. hash kernels
def _hash_call(kind, n, num_bins, salt, values=None):
  """ids / bytes hash (``num_bins`` None: the fingerprint) of periodic values into a guarded int64 buffer."""
  lib = _L()
  out = Guarded((n,), torch.int64)
  if kind == "bytes":
    blob, offsets = (_t(a) for a in hb.pack_periodic(hb.base_strings(), n))
    if num_bins is None:
      rc = lib.load().tfrs_fingerprint_bytes(lib.ptr(blob), lib.ptr(offsets), n, lib.ptr(out.view), lib.current_stream())
    else:
      rc = lib.load().tfrs_hash_bucket_strong_bytes(lib.ptr(blob), lib.ptr(offsets), n, num_bins, salt[0], salt[1],
                                                    lib.ptr(out.view), lib.current_stream())
  else:
    ids = _t(hb.base_ids(kind)[np.arange(n) % hb.PERIOD] if values is None else values)
    rc = lib.load().tfrs_hash_bucket_strong_ids(lib.ptr(ids), 1 if ids.dtype == torch.int64 else 0, n, num_bins,
                                                salt[0], salt[1], lib.ptr(out.view), lib.current_stream())
  torch.cuda.synchronize()
  assert rc == lib.TFRS_OK, lib.last_error()
  out.assert_guards("out")
  return out.view


@pytest.mark.parametrize("kind,num_bins,salt", [("i32", 1_000_003, (2, 1)), ("i64", 2 ** 62 + 7, (2 ** 63 + 5, 2 ** 64 - 1)),
                                                ("bytes", 1009, (4, 2)), ("bytes", None, None)])
def test_hash_kernels_past_the_grid_cap(kind, num_bins, salt):
  from tests import vocab_restatement as vr
  n = hb.N_HASH_PAST_CAP
  got = _hash_call(kind, n, num_bins, salt)
  _same_bits(got, hb.hash_expected(kind, n, num_bins, salt if salt else vr.FINGERPRINT_KEY))
  assert int(got[n - 1]) != I64_SENT and int(got[hb.HASH_CAP_BLOCKS * hb.BLOCK]) != I64_SENT


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("num_bins", hb.TOP_BINS)
def test_hash_ids_at_the_top_of_num_bins(num_bins, dtype):
  ids = hb.edge_ids(dtype)
  salt = (2 ** 63 + 5, 2 ** 64 - 1)
  got = _hash_call("i32" if dtype == np.int32 else "i64", ids.size, num_bins, salt, values=ids)
  want = o_hash.hash_bucket_strong(ids, num_bins, salt)
  assert want.max() > 2 ** 31 or num_bins == 3
  _same_bits(got, want)


# ================================================================================================ D. row hash
def _row_hash(rows_t, n, d):
  lib = _L()
  out = Guarded((n,), torch.int64)
  rc = lib.load().tfrs_row_hash64(lib.ptr(rows_t), n, d, lib.ptr(out.view), lib.current_stream())
  torch.cuda.synchronize()
  assert rc == lib.TFRS_OK, lib.last_error()
  out.assert_guards("out")
  return _np(out.view)


def _check_row_hashes(h, corpus, scalar):
  assert np.array_equal(h, hb.row_hash_np(corpus, scalar=scalar))
  assert (h >= 0).all()
  assert len({int(h[r]) for r in hb.PLANTED}) == 1
  for name, (a, b) in hb.PAIRS.items():
    assert h[a] != h[b], name


@pytest.mark.parametrize("d", hb.ROW_DIMS)
def test_row_hash_every_layout(d):
  corpus = hb.row_corpus(d)
  rows_t = _t(corpus)
  kind, _ = hb.row_hash_route(d, rows_t.data_ptr(), hb.ROW_N)
  assert kind == hb.row_hash_route(d)[0]
  _check_row_hashes(_row_hash(rows_t, hb.ROW_N, d), corpus, scalar=(kind == "scalar"))


def test_row_hash_from_a_base_that_is_not_16_byte_aligned():
  corpus = hb.row_corpus(64)
  flat = torch.zeros((corpus.size + 1,), dtype=torch.float32, device="cuda")
  flat[1:] = _t(corpus).reshape(-1)
  rows_t = flat[1:].view(corpus.shape)
  assert hb.row_hash_route(64, rows_t.data_ptr(), hb.ROW_N) == ("scalar", 1)
  scalar = _row_hash(rows_t, hb.ROW_N, 64)
  _check_row_hashes(scalar, corpus, scalar=True)
  aligned = _row_hash(_t(corpus), hb.ROW_N, 64)
  _check_row_hashes(aligned, corpus, scalar=False)
  assert (scalar != aligned).any()


@pytest.mark.parametrize("d", hb.DEDUP_DIMS)
def test_dedup_index_finds_the_planted_copies(d):
  import recommenders_amd as tfrs
  c, q = (a.copy() for a in hb.dedup_corpus(d))
  layer = tfrs.layers.factorized_top_k.BruteForce(k=5, dedup=True).index(c)
  assert layer._dup is not None and layer._dup.count == len(np.unique(c, axis=0))
  scores, rows = layer(q)
  want_scores, want_rows = o_topk.brute_force(q, c, 5)
  np.testing.assert_array_equal(_np(rows), want_rows)
  np.testing.assert_array_equal(_np(scores), want_scores)
