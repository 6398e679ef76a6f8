"""Hand-built inputs and plain restatements for the integer kernels in front of the embedding tables (no test
functions; imported by ``test_ids_handbuilt_host.py``, which proves on the host that every case has the property
it is named for, and by ``test_ids_layout_gpu.py``, which runs the kernels on them).

  A. ``csrc/shard_route.hip``: ``route`` is the stable bucket sort by owner; ``route_by_tiles`` restates the
     three kernels' own decomposition (4096-id tiles, 64 lanes x ``per`` tiles x chunks of 8 in the scan,
     64-id segments in the placement) so that a wrong variant of one step can be stated and shown to differ.
  B. ``csrc/hashing.hip``, fused lookups: tables whose cells name (table, row, column), periodic ids, the
     expected ``out`` / ``buckets`` built launch by launch the way the entry points split their work.
  C. ``csrc/hashing.hip``, hash kernels: periodic ids / packed strings past the grid cap, Barrett reduction.
  D. ``csrc/dedup.hip``: both row-hash kernels in Python ints and in NumPy ``uint64``, the dispatch rule.

Everything is integer work (the table cells are integers below 2^24, exact in float32): every comparison
built on this module is exact.  SipHash comes from ``oracle/hashing.py``."""

import functools

import numpy as np

from oracle import hashing as o_hash

U64 = (1 << 64) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def frozen(a):
  a = np.ascontiguousarray(a)
  a.setflags(write=False)
  return a


# ======================================================================== A. shard routing
TILE, SEG, SCAN_LANES, SCAN_CHUNK, MAX_WORLD = 4096, 64, 64, 8, 64


def workspace_bytes(n, world):
  """``tfrs_shard_route_workspace_bytes``: tile_base (int64) + tile_counts (uint32) per (tile, owner) + 256."""
  if n <= 0 or world <= 0:
    return 256
  return -(-n // TILE) * world * (8 + 4) + 256


def scan_shape(n):
  """How ``shard_scan_kernel`` cuts ``n`` ids: (ntiles, per, [(t0, t1)] per lane).  A lane's range is empty
  when t0 >= t1."""
  ntiles = -(-n // TILE)
  per = -(-ntiles // SCAN_LANES)
  ranges = [(lane * per, min(lane * per + per, ntiles)) for lane in range(SCAN_LANES)]
  return ntiles, per, ranges


def lane_chunks(t0, t1):
  """(full chunks of 8 tiles, tiles of the partial chunk behind them) of one lane's range."""
  tiles = max(t1 - t0, 0)
  return tiles // SCAN_CHUNK, tiles % SCAN_CHUNK


def owner_local(ids, input_dim, rows_per_rank):
  """(owner, shard-local row) of every id; an id outside [0, input_dim) goes to owner 0 as row -1."""
  ids = np.asarray(ids).astype(np.int64)
  valid = (ids >= 0) & (ids < input_dim)
  safe = np.where(valid, ids, 0)
  owner = safe // rows_per_rank
  local = np.where(valid, safe - owner * rows_per_rank, -1)
  return owner.astype(np.int64), local.astype(np.int64)


def route(ids, input_dim, rows_per_rank, world):
  """The operation: a stable bucket sort by owner -> (send_ids int64, perm int32, order int32, counts int64)."""
  owner, local = owner_local(ids, input_dim, rows_per_rank)
  order = np.argsort(owner, kind="stable")
  perm = np.empty(order.size, dtype=np.int32)
  perm[order] = np.arange(order.size, dtype=np.int32)
  return local[order], perm, order.astype(np.int32), np.bincount(owner, minlength=world).astype(np.int64)


def tile_counts(owner, world):
  """[ntiles, world]: ids per owner in every 4096-id tile (``shard_count_kernel``)."""
  ntiles = -(-owner.size // TILE)
  key = (np.arange(owner.size) // TILE) * world + owner
  return np.bincount(key, minlength=ntiles * world).reshape(ntiles, world).astype(np.int64)


def segment_counts(owner, world):
  """[nsegments, world]: ids per owner in every 64-id segment (pass 1 of ``shard_place_kernel``)."""
  nseg = -(-owner.size // SEG)
  key = (np.arange(owner.size) // SEG) * world + owner
  return np.bincount(key, minlength=nseg * world).reshape(nseg, world).astype(np.int64)


def scan_tiles(counts, drop_partial_chunk=False):
  """``shard_scan_kernel`` lane by lane: (tile_base [ntiles, world], totals [world]).  Lane l sums its range, the
  exclusive scan of the 64 sums starts its running position, and the lane rewrites its range in chunks of 8.
  ``drop_partial_chunk`` is the WRONG scan that only handles full chunks: the tiles of a partial chunk keep a
  base of 0 and do not advance the running position."""
  ntiles, world = counts.shape
  _, _, ranges = scan_shape(ntiles * TILE)
  base = np.zeros((ntiles, world), dtype=np.int64)
  sums = np.stack([counts[t0:t1].sum(axis=0) if t0 < t1 else np.zeros(world, np.int64) for t0, t1 in ranges])
  incl = np.cumsum(sums, axis=0)
  for lane, (t0, t1) in enumerate(ranges):
    run = incl[lane] - sums[lane]
    for tb in range(t0, t1, SCAN_CHUNK):
      stop = min(tb + SCAN_CHUNK, t1)
      if drop_partial_chunk and stop - tb < SCAN_CHUNK:
        continue
      chunk = counts[tb:stop]
      base[tb:stop] = run + np.cumsum(chunk, axis=0) - chunk
      run = run + chunk.sum(axis=0)
  return base, incl[-1]


def route_by_tiles(ids, input_dim, rows_per_rank, world, drop_partial_chunk=False, unstable_in_segment=False):
  """The three kernels' decomposition: position = owner's start + tile base + ids of the same owner before it in
  its tile.  With both flags off this IS ``route`` (shown by the host test).  ``unstable_in_segment`` is the WRONG
  placement that ranks the ids of one owner inside a 64-id segment from the segment's end."""
  owner, local = owner_local(ids, input_dim, rows_per_rank)
  n = owner.size
  base, totals = scan_tiles(tile_counts(owner, world), drop_partial_chunk)
  start = np.cumsum(totals) - totals
  i = np.arange(n)
  within = i % SEG
  if unstable_in_segment:
    within = SEG - 1 - within
  # rank inside the tile among the ids of the same owner: segments in order, lanes by `within`
  by = np.lexsort((within, i // SEG, owner, i // TILE))
  key = (i // TILE) * world + owner
  skey = key[by]
  first = np.r_[True, skey[1:] != skey[:-1]]
  group_start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
  rank = np.empty(n, dtype=np.int64)
  rank[by] = np.arange(n) - group_start
  pos = start[owner] + base[i // TILE, owner] + rank
  send = np.full(n, np.iinfo(np.int64).min, dtype=np.int64)
  order = np.full(n, -1, dtype=np.int32)
  ok = (pos >= 0) & (pos < n)          # (a wrong variant may point outside; such a write is left out here)
  send[pos[ok]] = local[ok]
  order[pos[ok]] = i[ok].astype(np.int32)
  return send, pos.astype(np.int32), order, totals.astype(np.int64)


N_PER9 = 513 * TILE - 5            # 513 tiles, per = 9: lanes 0..56 hold 8 + 1 tiles, lanes 57..63 nothing
N_PER17 = 1030 * TILE + 77         # 1031 tiles, per = 17: lanes 0..59 hold 8 + 8 + 1, lane 60 8 + 3, 61..63 nothing
N_PER1 = 64 * TILE                 # one full tile in every lane
N_PER2 = 64 * TILE + 1             # per = 2: lane 32 holds one tile of one id, lanes 33..63 nothing
N_MID = 3 * TILE + 1000            # a few tiles and a tail
SCAN_NS = (N_PER9, N_PER17, N_PER1, N_PER2, 63, 64, 65, 4095, 4096)
DIM, WORLD = 1_000_003, 8          # the default geometry: 8 ranks, a table that is no multiple of the world
RPR = -(-DIM // WORLD)


class RouteCase:
  """ids (int64, read-only) with their geometry; ``fits32`` when every id is an int32 value."""

  def __init__(self, name, ids, input_dim=DIM, rows_per_rank=RPR, world=WORLD):
    self.name, self.input_dim, self.rows_per_rank, self.world = name, int(input_dim), int(rows_per_rank), int(world)
    self.ids = frozen(np.asarray(ids, dtype=np.int64))
    self.n = self.ids.size
    self.fits32 = bool(self.n == 0 or (self.ids.min() >= INT32_MIN and self.ids.max() <= INT32_MAX))

  @functools.cached_property
  def expected(self):
    return tuple(frozen(a) for a in route(self.ids, self.input_dim, self.rows_per_rank, self.world))


def _in_owner(owner, n, rows_per_rank=RPR, input_dim=DIM):
  """An id of ``owner`` for each of n positions: the local row walks through the owner's range."""
  owner = np.broadcast_to(np.asarray(owner, dtype=np.int64), (n,))
  top = np.minimum((owner + 1) * rows_per_rank, input_dim) - owner * rows_per_rank     # rows the owner really has
  return owner * rows_per_rank + (np.arange(n, dtype=np.int64) * 7919) % top


def _random_ids(n, seed):
  rng = np.random.default_rng(seed)
  ids = rng.integers(0, DIM, size=n)
  if n > 10:
    ids[3], ids[7], ids[n // 2], ids[n - 1] = -5, DIM, INT32_MAX, DIM - 1
  return ids


def _runs(n, length, shift):
  """Owner runs of ``length`` ids; the owner of run r is (5 r + 3) mod 8; ``shift`` moves the cuts."""
  run = (np.arange(n) + shift) // length
  return (5 * run + 3) % WORLD


INVALID_32 = (-1, DIM, INT32_MIN, INT32_MAX, -DIM, DIM + 1)
INVALID_64 = INVALID_32 + (INT64_MIN, INT64_MAX, 1 << 40, -(1 << 40))


def _invalid_tile(n, wide):
  """Uniform ids with tile 1 (ids 4096..8191) made of ids outside the table only."""
  ids = _random_ids(n, 77)
  bad = np.asarray(INVALID_64 if wide else INVALID_32, dtype=np.int64)
  ids[TILE:2 * TILE] = bad[np.arange(TILE) % bad.size]
  return ids


def _pattern_builders(tag, n):
  i = np.arange
  b = {f"all_owner0@{tag}": lambda: _in_owner(0, n),
       f"all_last_owner@{tag}": lambda: _in_owner(WORLD - 1, n),
       f"all_owner5@{tag}": lambda: _in_owner(5, n),
       f"alternating_2_6@{tag}": lambda: _in_owner(np.where(i(n) % 2 == 0, 2, 6), n)}
  for length in (SEG, TILE):
    for shift in (0, 1):
      b[f"runs{length}+{shift}@{tag}"] = lambda length=length, shift=shift: _in_owner(_runs(n, length, shift), n)
  b[f"invalid_tile32@{tag}"] = lambda: _invalid_tile(n, False)
  b[f"invalid_tile64@{tag}"] = lambda: _invalid_tile(n, True)
  b[f"owners_1_4_6_only@{tag}"] = lambda: _in_owner(np.asarray([1, 4, 6])[(i(n) * i(n) + i(n) // 3) % 3], n)
  return {k: (lambda f=f: (f(),)) for k, f in b.items()}


def _world_case(world):
  rng = np.random.default_rng(world)
  ids = rng.integers(0, DIM, size=N_MID)
  ids[[0, 5, N_MID - 1]] = [-1, DIM, DIM - 1]
  return ids, DIM, -(-DIM // world), world


def _table_2_40():
  """A table beyond 2^31 (and 2^40) rows: ids in the last rows of the last ranks, and one past the end."""
  i = np.arange(N_MID)
  big = (1 << 40) + 3
  rpr = -(-big // 64)
  near_top = big - 1 - (i % 1000) * (rpr // 400)
  near_top[::97] = big
  near_top[1::97] = (1 << 40) - (i[1::97] % 5)
  return near_top, big, rpr, 64


def _geometry_builders():
  n, i = N_MID, np.arange(N_MID)
  b = {f"world{w}": functools.partial(_world_case, w) for w in (1, 2, 63, 64)}
  # 1000 rows, 500 per rank, 8 ranks: ranks 2..7 own no row
  b["trailing_ranks_empty"] = lambda: (np.random.default_rng(6).integers(-2, 1002, size=n), 1000, 500, 8)
  # one row per rank: 64 ranks, and 40 rows over 64 ranks (24 trailing ranks without a row)
  b["one_row_per_rank"] = lambda: ((i * 37) % 64, 64, 1, 64)
  b["one_row_per_rank_40_of_64"] = lambda: (np.random.default_rng(7).integers(-1, 41, size=n), 40, 1, 64)
  b["table_2^40"] = _table_2_40
  b["one_row_one_rank"] = lambda: (np.where(i % 3 == 0, 0, np.where(i % 3 == 1, 1, -1)), 1, 1, 1)
  b["one_row_four_ranks"] = lambda: (np.where(i % 5 == 0, 1, 0), 1, 1, 4)
  return b


ROUTE_BUILDERS = {f"scan_n{n}": (lambda n=n: (_random_ids(n, n),)) for n in SCAN_NS}
ROUTE_BUILDERS.update(_pattern_builders("mid", N_MID))
ROUTE_BUILDERS.update(_pattern_builders("per17", N_PER17))
ROUTE_BUILDERS.update(_geometry_builders())
ROUTE_NAMES = tuple(ROUTE_BUILDERS)
ROUTE_WIDE = ("invalid_tile64@mid", "invalid_tile64@per17", "table_2^40")     # ids that are no int32 values


@functools.lru_cache(maxsize=2)
def route_case(name):
  """The case of that name (built on demand: the large ones hold 4 M ids each)."""
  return RouteCase(name, *ROUTE_BUILDERS[name]())


# ======================================================================== B / C. hashing and the fused lookups
HASH_CAP_BLOCKS, LOOKUP_CAP_BLOCKS, BLOCK = 8192, 4096, 256     # hash_grid(); the fused lookups' grid
MAX_CHUNKS, MAX_UNITS = 16, 64                                   # descriptors of one launch
PERIOD = 211                                                     # a prime: ids[v] = base[v % 211]
N_HASH_PAST_CAP = HASH_CAP_BLOCKS * BLOCK + 300
N_LOOKUP_PAST_CAP = 65_537                                       # x 16 chunks (units) = 1 048 592 lookups
DIMS = (4, 8, 16, 32, 64, 128, 256)
TOP_BINS = ((1 << 63) - 1, 1 << 32, (1 << 32) + 1, 3)


def barrett(h, m):
  """``mod_barrett`` in Python ints: (remainder, conditional subtractions used, the estimate's deficit)."""
  recip = U64 // m
  q = (h * recip) >> 64
  r = h - q * m
  assert 0 <= r <= U64
  used = 0
  for _ in range(2):
    if r >= m:
      r -= m
      used += 1
  return r, used, h // m - q


def edge_ids(dtype):
  """The edge id list of ``test_hash_ids_parity``."""
  info = np.iinfo(dtype)
  edge = [0, 1, -1, 9, 10, 99, 100, 12345678, 99999999, 100000000, info.max, info.min, info.max - 1, info.min + 1]
  edge += [10 ** k for k in range(1, 19) if 10 ** k <= info.max]
  edge += [-(10 ** k) for k in range(1, 19) if 10 ** k <= info.max]
  return np.asarray(edge, dtype=dtype)


@functools.lru_cache(maxsize=None)
def base_ids(kind):
  """PERIOD ids of ``kind`` 'i32' / 'i64': the edge list first, then random ones over the type's range."""
  dtype = np.int32 if kind == "i32" else np.int64
  rng = np.random.default_rng(31 if kind == "i32" else 63)
  edge = edge_ids(dtype)
  info = np.iinfo(dtype)
  small = rng.integers(0, 10_000_000, size=(PERIOD - edge.size) // 2).astype(dtype)
  rest = rng.integers(info.min, info.max, size=PERIOD - edge.size - small.size, dtype=dtype)
  ids = np.concatenate([edge, small, rest])
  assert ids.size == PERIOD
  return frozen(ids)


@functools.lru_cache(maxsize=None)
def base_strings():
  """PERIOD byte strings: every length 0 .. 40 (the 8-byte word edges 7, 8, 9, 15, 16, 17 among them), then
  random lengths up to 70; bytes over the whole range, so sign extension of a byte would show."""
  rng = np.random.default_rng(8)
  lens = list(range(41)) + rng.integers(0, 71, size=PERIOD - 41).tolist()
  return tuple(bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist()) for n in lens)


def base_values(kind):
  return base_strings() if kind == "bytes" else [int(x) for x in base_ids(kind)]


@functools.lru_cache(maxsize=None)
def sip_column(kind, salt0, salt1):
  """Unsigned SipHash-2-4 under (salt0, salt1) of the PERIOD base values of ``kind`` (a tuple of Python ints)."""
  return tuple(o_hash.siphash24(salt0, salt1, v if kind == "bytes" else str(v).encode("ascii"))
               for v in base_values(kind))


def as_signed(u):
  return u - (1 << 64) if u >= (1 << 63) else u


def pack_periodic(strings, n):
  """(blob uint8, offsets int64[n + 1]) of n strings, string i = strings[i % len(strings)], built with NumPy."""
  p = len(strings)
  lens = np.asarray([len(s) for s in strings], dtype=np.int64)
  offsets = np.zeros(n + 1, dtype=np.int64)
  np.cumsum(lens[np.arange(n) % p], out=offsets[1:])
  period = np.frombuffer(b"".join(strings), dtype=np.uint8)
  tail = np.frombuffer(b"".join(strings[:n % p]), dtype=np.uint8)
  blob = np.concatenate([np.tile(period, n // p), tail])
  assert blob.size == offsets[-1]
  return (blob if blob.size else np.zeros(1, np.uint8)), offsets


def salt_of(unit):
  """(salt0, salt1) of chunk / unit number ``unit``: salt0 uses all 64 bits, salt1 is the number."""
  return ((unit + 1) * 0x9E3779B97F4A7C15) & U64, unit


def table_of(unit):
  """Units 2, 5, 8, ... read the table of the unit two before them; every other unit has a table of its own."""
  return unit - 2 if unit % 3 == 2 else unit


def cell_values(tables, rows, d):
  """float32 [..., d]: cell (table, row, column) holds (table * 256 + row) * 256 + column < 2^24."""
  tables, rows = np.asarray(tables, dtype=np.int64), np.asarray(rows, dtype=np.int64)
  v = ((tables * 256 + rows)[..., None] * 256 + np.arange(d)).astype(np.float32)
  return v


def make_table(unit, num_bins, d):
  assert table_of(unit) == unit and unit < 256 and num_bins <= 256 and d <= 256
  return cell_values(np.full(num_bins, unit), np.arange(num_bins), d)


def lookup_launches(n_slots, per_launch):
  """[(first chunk / unit, count)] of the launches ``n_slots`` chunks (units) take."""
  return [(c0, min(per_launch, n_slots - c0)) for c0 in range(0, n_slots, per_launch)]


def last_wave(total, cap_blocks):
  """(lookups past the first grid-stride pass, live lanes of the last wave) of ``total`` one-lane items on a grid
  of min(ceil(total / 256), cap_blocks) blocks."""
  blocks = max(1, min(-(-total // BLOCK), cap_blocks))
  return max(total - blocks * BLOCK, 0), (total % 64) or 64


def unit_buckets(kind, n_values, units, num_bins, rotate=None):
  """int64 [n_values, len(units)]: bucket of value v under unit u's salt; value v is base[(v + rotate[u]) % PERIOD]."""
  cols = np.empty((PERIOD, len(units)), dtype=np.int64)
  for k, u in enumerate(units):
    cols[:, k] = [h % num_bins for h in sip_column(kind, *salt_of(u))]
  v = np.arange(n_values)[:, None] + (np.zeros(len(units), np.int64) if rotate is None else np.asarray(rotate))[None, :]
  return cols[v % PERIOD, np.arange(len(units))[None, :]]


def unified_expected(kind, n_values, n_chunks, num_bins, d, sentinel, ignore_chunk0=False):
  """(out float32 [n, C * d], buckets int64 [n, C]) of ``tfrs_unified_embedding_fwd``, written launch by launch into
  buffers of ``sentinel``.  ``ignore_chunk0`` is the WRONG kernel that forgets ``out_chunk0``: every launch writes
  from column block 0."""
  out = np.full((n_values, n_chunks, d), sentinel, dtype=np.float32)
  buckets = np.full((n_values, n_chunks), int(sentinel), dtype=np.int64)
  b = unit_buckets(kind, n_values, range(n_chunks), num_bins)
  for c0, cl in lookup_launches(n_chunks, MAX_CHUNKS):
    at = 0 if ignore_chunk0 else c0
    tabs = np.asarray([table_of(c) for c in range(c0, c0 + cl)])
    out[:, at:at + cl] = cell_values(np.broadcast_to(tabs, (n_values, cl)), b[:, c0:c0 + cl], d)
    buckets[:, at:at + cl] = b[:, c0:c0 + cl]
  return out.reshape(n_values, n_chunks * d), buckets


FEATURE_CHUNKS = (1, 3, 2, 5)      # chunk counts of consecutive features, cycled


def multi_layout(n_units):
  """Units of a multi call: consecutive features with 1, 3, 2, 5, 1, ... chunks; the last feature is cut where
  the units run out (its remaining column blocks are never written).  -> (feature of unit, chunk index of unit,
  declared chunks per feature)."""
  feature, chunk, declared = [], [], []
  while len(feature) < n_units:
    c = FEATURE_CHUNKS[len(declared) % len(FEATURE_CHUNKS)]
    declared.append(c)
    for k in range(min(c, n_units - len(feature))):
      feature.append(len(declared) - 1)
      chunk.append(k)
  return feature, chunk, declared


def multi_ids(kind, n_values, feature):
  """ids of feature f: base[(v + 7 f) % PERIOD]."""
  return base_ids(kind)[(np.arange(n_values) + 7 * feature) % PERIOD]


def multi_expected(kind, n_values, n_units, num_bins, d, sentinel):
  """([out float32 [n, chunks_f * d] per feature], buckets int64 [n, n_units]) of
  ``tfrs_unified_embedding_fwd_multi``."""
  feature, chunk, declared = multi_layout(n_units)
  b = unit_buckets(kind, n_values, range(n_units), num_bins, rotate=[7 * f for f in feature])
  outs = [np.full((n_values, c, d), sentinel, dtype=np.float32) for c in declared]
  for u in range(n_units):
    outs[feature[u]][:, chunk[u]] = cell_values(np.full(n_values, table_of(u)), b[:, u], d)
  return [o.reshape(n_values, -1) for o in outs], b


def hash_expected(kind, n, num_bins, salt, stop_at=None, sentinel=0):
  """int64 [n]: ``hash mod num_bins`` of value i % PERIOD (``num_bins`` None: the raw hash as int64).  ``stop_at``
  is the WRONG kernel without a grid-stride loop: items from ``stop_at`` on keep ``sentinel``."""
  col = sip_column(kind, *salt)
  ref = np.asarray([as_signed(h) if num_bins is None else h % num_bins for h in col], dtype=np.int64)
  out = ref[np.arange(n) % PERIOD]
  if stop_at is not None:
    out[stop_at:] = sentinel
  return out


# ======================================================================== D. row hash
GOLD, MIX1, MIX2, MASK63 = 0x9E3779B97F4A7C15, 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53, (1 << 63) - 1
ROW_DIMS = (4, 8, 12, 20, 100, 128, 256, 7, 1)
ROW_N = 333                        # 333 * LPR is no multiple of 64 for LPR = 1 .. 32: a partly empty last wave
PLANTED = (0, 1, 63, 64, ROW_N - 1)
PAIRS = {"last_word": (2, 3), "first_word": (4, 5), "signed_zero": (6, 7)}


def mix64(h):
  h ^= h >> 33
  h = (h * MIX1) & U64
  h ^= h >> 33
  h = (h * MIX2) & U64
  h ^= h >> 33
  return h


def row_hash_route(d, base_address=0, n=1):
  """('pieces', lanes per row) or ('scalar', 1): the dispatch rule of ``tfrs_row_hash64``."""
  if d % 4 == 0 and base_address % 16 == 0 and n * 64 < (1 << 39):
    pieces = d // 4
    return "pieces", max(l for l in (1, 2, 4, 8, 16, 32) if l <= pieces)
  return "scalar", 1


def row_hash_int(words, lanes=None):
  """One row (a list of uint32 words) in Python ints, lane by lane like the kernel ``tfrs_row_hash64`` picks."""
  d = len(words)
  kind, lpr = row_hash_route(d) if lanes is None else lanes
  if kind == "scalar":
    h = GOLD ^ d
    for w in words:
      h ^= (w + GOLD + (h << 6) + (h >> 2)) & U64
      h = (h * MIX1) & U64
      h ^= h >> 33
    return h & MASK63
  pieces, lane_sum = d // 4, []
  for lane in range(lpr):
    h = 0
    for c in range(lane, pieces, lpr):
      x, y, z, w = words[4 * c:4 * c + 4]
      k = ((c + 1) * GOLD) & U64
      a, b = (y << 32) | x, (w << 32) | z
      h = (h + mix64(a ^ k) + mix64((b + (((k << 1) & U64) | 1)) & U64)) & U64
    lane_sum.append(h)
  return mix64((sum(lane_sum) & U64) ^ d) & MASK63


def _mix64_np(h):
  h = h ^ (h >> np.uint64(33))
  h = h * np.uint64(MIX1)
  h = h ^ (h >> np.uint64(33))
  h = h * np.uint64(MIX2)
  return h ^ (h >> np.uint64(33))


def row_hash_np(rows, scalar=False):
  """int64 [n]: the hash of every float32 row, NumPy ``uint64`` (wrapping) arithmetic."""
  rows = np.ascontiguousarray(rows, dtype=np.float32)
  n, d = rows.shape
  w = rows.view(np.uint32).astype(np.uint64)
  with np.errstate(over="ignore"):
    if scalar or d % 4 != 0:
      h = np.full(n, GOLD ^ d, dtype=np.uint64)
      for k in range(d):
        h = h ^ (w[:, k] + np.uint64(GOLD) + (h << np.uint64(6)) + (h >> np.uint64(2)))
        h = h * np.uint64(MIX1)
        h = h ^ (h >> np.uint64(33))
    else:
      w = w.reshape(n, d // 4, 4)
      key = np.asarray([((c + 1) * GOLD) & U64 for c in range(d // 4)], dtype=np.uint64)
      key2 = (key << np.uint64(1)) | np.uint64(1)
      a = (w[:, :, 1] << np.uint64(32)) | w[:, :, 0]
      b = (w[:, :, 3] << np.uint64(32)) | w[:, :, 2]
      h = (_mix64_np(a ^ key) + _mix64_np(b + key2)).sum(axis=1, dtype=np.uint64)
      h = _mix64_np(h ^ np.uint64(d))
    return (h & np.uint64(MASK63)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def row_corpus(d):
  """float32 [ROW_N, d]: random rows; one row planted at PLANTED; the PAIRS differ only in the last word, only
  in the first word, and only by +0.0 against -0.0 in the middle word."""
  rng = np.random.default_rng(1000 + d)
  c = rng.normal(size=(ROW_N, d)).astype(np.float32)
  c[list(PLANTED)] = c[0]
  for a, b in PAIRS.values():
    c[b] = c[a]
  a, b = PAIRS["last_word"]
  c[b, d - 1] = np.nextafter(c[a, d - 1], np.float32(np.inf))
  a, b = PAIRS["first_word"]
  c[b, 0] = np.nextafter(c[a, 0], np.float32(np.inf))
  a, b = PAIRS["signed_zero"]
  c[a, d // 2], c[b, d // 2] = 0.0, -0.0
  return frozen(c)


DEDUP_DIMS = (4, 12, 100, 128, 7)


@functools.lru_cache(maxsize=None)
def dedup_corpus(d):
  """(corpus float32 [600, d] with planted copies, queries float32 [9, d])."""
  rng = np.random.default_rng(2000 + d)
  base = (rng.normal(size=(450, d)) / np.sqrt(d)).astype(np.float32)
  pick = np.concatenate([np.arange(450), rng.integers(0, 40, size=150)])
  c = base[rng.permutation(pick)]
  q = (rng.normal(size=(9, d)) / np.sqrt(d)).astype(np.float32)
  return frozen(c), frozen(q)
