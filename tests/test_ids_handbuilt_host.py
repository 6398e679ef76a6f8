"""Host proofs for tests/ids_handbuilt.py (no GPU): every hand-built case of tests/test_ids_layout_gpu.py has the
property it is named for, the restatements agree with each other and with values worked out by hand, and for
every edge a deliberately WRONG variant of the restatement gives a different expected output on the case built for
it -- so a kernel with that fault cannot pass the GPU file."""

import numpy as np
import pytest

from oracle import hashing as o_hash
from tests import ids_handbuilt as hb


class _Cases:
  """The routing cases by name, built on demand (``hb.route_case`` keeps the last two)."""

  def __getitem__(self, name):
    return hb.route_case(name)

  def values(self):
    return (hb.route_case(name) for name in hb.ROUTE_NAMES)


CASES = _Cases()


# ---- A. shard routing ------------------------------------------------------------------------------------------
def test_route_case_names():
  assert len(hb.ROUTE_NAMES) == 9 + 2 * 11 + 10 and set(hb.ROUTE_WIDE) < set(hb.ROUTE_NAMES)


def _lanes(n):
  ntiles, per, ranges = hb.scan_shape(n)
  return ntiles, per, [hb.lane_chunks(t0, t1) for t0, t1 in ranges]


def test_scan_shapes_are_what_they_are_named_for():
  ntiles, per, lanes = _lanes(hb.N_PER9)
  assert (ntiles, per) == (513, 9) and lanes == [(1, 1)] * 57 + [(0, 0)] * 7
  assert hb.N_PER9 % hb.TILE == hb.TILE - 5                     # a last tile that is 5 ids short
  ntiles, per, lanes = _lanes(hb.N_PER17)
  assert (ntiles, per) == (1031, 17) and lanes == [(2, 1)] * 60 + [(1, 3)] + [(0, 0)] * 3
  assert hb.N_PER17 % hb.TILE == 77
  ntiles, per, lanes = _lanes(hb.N_PER1)
  assert (ntiles, per) == (64, 1) and lanes == [(0, 1)] * 64 and hb.N_PER1 % hb.TILE == 0
  ntiles, per, lanes = _lanes(hb.N_PER2)
  assert (ntiles, per) == (65, 2) and lanes == [(0, 2)] * 32 + [(0, 1)] + [(0, 0)] * 31
  assert hb.N_PER2 - 64 * hb.TILE == 1                          # the last lane with work: one tile of one id
  for n in (63, 64, 65, 4095, 4096):
    assert _lanes(n)[:2] == (1, 1)
  assert _lanes(hb.N_MID)[:2] == (4, 1) and hb.N_MID % hb.TILE == 1000 and hb.N_MID % hb.SEG == 40
  # what the suite had before: at most per = 2, never a second chunk of 8
  assert _lanes(300_000)[1] == 2
  assert {CASES[f"scan_n{n}"].n for n in hb.SCAN_NS} == set(hb.SCAN_NS)


def _counts(case):
  owner, local = hb.owner_local(case.ids, case.input_dim, case.rows_per_rank)
  return owner, local, hb.segment_counts(owner, case.world), hb.tile_counts(owner, case.world)


@pytest.mark.parametrize("tag,n", [("mid", hb.N_MID), ("per17", hb.N_PER17)])
def test_owner_patterns_are_what_they_are_named_for(tag, n):
  full_segs, full_tiles = n // hb.SEG, n // hb.TILE
  for name, o in (("all_owner0", 0), ("all_last_owner", 7), ("all_owner5", 5)):
    case = CASES[f"{name}@{tag}"]
    owner, local, seg, tile = _counts(case)
    assert case.n == n and (owner == o).all() and (local >= 0).all()
    assert (seg[:full_segs, o] == 64).all() and (tile[:full_tiles, o] == 4096).all()
    assert case.expected[3].tolist() == [n if r == o else 0 for r in range(8)]
  owner, _, seg, tile = _counts(CASES[f"alternating_2_6@{tag}"])
  assert (owner[0::2] == 2).all() and (owner[1::2] == 6).all()
  assert (seg[:full_segs, 2] == 32).all() and (seg[:full_segs, 6] == 32).all()
  for length, counts_of in ((64, 1), (4096, 2)):
    owner, _, *counts = _counts(CASES[f"runs{length}+0@{tag}"])
    c = counts[counts_of - 1]
    assert set(np.unique(c[:n // length])) == {0, length}        # every segment / tile belongs to ONE owner
    assert len(np.unique(owner)) == min(8, -(-n // length))
    owner1, _, *counts1 = _counts(CASES[f"runs{length}+1@{tag}"])
    c1 = counts1[counts_of - 1]
    full = c1[1:n // length - 1]                                   # shifted: every segment / tile is cut 1 : length - 1
    assert sorted(np.unique(full)) == [0, 1, length - 1]
    assert (owner1[:-1] == owner[1:]).all()
  for wide in ("32", "64"):
    case = CASES[f"invalid_tile{wide}@{tag}"]
    owner, local, seg, tile = _counts(case)
    bad = case.ids[hb.TILE:2 * hb.TILE]
    assert ((bad < 0) | (bad >= case.input_dim)).all() and (local[hb.TILE:2 * hb.TILE] == -1).all()
    assert tile[1].tolist() == [4096] + [0] * 7
    assert case.fits32 == (wide == "32")
    want = hb.INVALID_64 if wide == "64" else hb.INVALID_32
    assert set(bad.tolist()) == set(want) and case.input_dim in want
    assert {hb.INT32_MIN, hb.INT32_MAX, -1} <= set(bad.tolist())
  assert {hb.INT64_MIN, hb.INT64_MAX} <= set(CASES[f"invalid_tile64@{tag}"].ids.tolist())
  counts = CASES[f"owners_1_4_6_only@{tag}"].expected[3]
  assert [r for r in range(8) if counts[r] > 0] == [1, 4, 6] and counts.sum() == n


def test_geometry_cases_are_what_they_are_named_for():
  assert [CASES[f"world{w}"].world for w in (1, 2, 63, 64)] == [1, 2, 63, 64]
  for w in (1, 2, 63, 64):
    case = CASES[f"world{w}"]
    assert (case.expected[3] > 0).all() and (case.expected[0] == -1).sum() == 2
  case = CASES["trailing_ranks_empty"]
  assert -(-case.input_dim // case.rows_per_rank) == 2 < case.world == 8
  assert (case.expected[3][:2] > 0).all() and (case.expected[3][2:] == 0).all()
  case = CASES["one_row_per_rank"]
  assert case.rows_per_rank == 1 and case.world == 64 and (case.expected[3] > 0).all() and (case.expected[0] == 0).all()
  case = CASES["one_row_per_rank_40_of_64"]
  assert (case.expected[3][:40] > 0).all() and (case.expected[3][40:] == 0).all() and (case.expected[0] == -1).any()
  case = CASES["table_2^40"]
  assert case.input_dim == 2 ** 40 + 3 and not case.fits32 and case.rows_per_rank * 63 < case.input_dim
  owner, local, _, _ = _counts(case)
  assert case.ids.max() == case.input_dim and (case.ids >= 2 ** 40 - 4).sum() > 100 and case.ids.min() > 2 ** 39
  assert owner.max() == 63 and local.max() > 2 ** 33 and (local == -1).any()     # local rows beyond 32 bits
  assert (case.ids == case.input_dim - 1).any()
  case = CASES["one_row_one_rank"]
  assert (case.input_dim, case.world) == (1, 1) and set(case.expected[0].tolist()) == {0, -1}
  case = CASES["one_row_four_ranks"]
  assert case.expected[3][1:].tolist() == [0, 0, 0] and set(case.expected[0].tolist()) == {0, -1}


def test_every_route_case_is_a_valid_call_and_a_permutation():
  for case in CASES.values():
    assert 1 <= case.world <= hb.MAX_WORLD and -(-case.input_dim // case.rows_per_rank) <= case.world
    send, perm, order, counts = case.expected
    assert send.dtype == np.int64 and perm.dtype == order.dtype == np.int32 and counts.dtype == np.int64
    assert counts.sum() == case.n and counts.size == case.world
    assert (order[perm] == np.arange(case.n)).all()
    assert (send >= -1).all() and (send < case.rows_per_rank).all()
    assert case.fits32 == (case.name not in hb.ROUTE_WIDE)


@pytest.mark.parametrize("name", ["scan_n4095", "scan_n65", "runs64+1@mid", "invalid_tile64@mid", "world63",
                                  "table_2^40", "scan_n%d" % hb.N_PER9, "owners_1_4_6_only@per17"])
def test_tile_decomposition_is_the_stable_bucket_sort(name):
  """count -> scan (64 lanes, chunks of 8) -> place by tile, segment and lane IS the stable sort by owner."""
  case = CASES[name]
  got = hb.route_by_tiles(case.ids, case.input_dim, case.rows_per_rank, case.world)
  for g, w in zip(got, case.expected):
    assert g.dtype == w.dtype and np.array_equal(g, w)


def test_route_on_a_list_small_enough_to_sort_by_hand():
  # 3 rows per rank, 3 ranks, 8 rows: owners 2 0 0 - 1 2 0, where "-" (id 8) is outside and goes to owner 0 as row -1
  send, perm, order, counts = hb.route([7, 0, 2, 8, 4, 6, 1], 8, 3, 3)
  assert order.tolist() == [1, 2, 3, 6, 4, 0, 5] and send.tolist() == [0, 2, -1, 1, 1, 1, 0]
  assert perm.tolist() == [5, 0, 1, 2, 4, 6, 3] and counts.tolist() == [4, 1, 2]


@pytest.mark.parametrize("name", ["alternating_2_6@mid", "runs64+1@mid", "scan_n65", "scan_n4096"])
def test_unstable_placement_inside_a_segment_is_told_apart(name):
  case = CASES[name]
  wrong = hb.route_by_tiles(case.ids, case.input_dim, case.rows_per_rank, case.world, unstable_in_segment=True)
  assert np.array_equal(wrong[3], case.expected[3])                # the counts cannot tell
  assert not np.array_equal(wrong[1], case.expected[1]) and not np.array_equal(wrong[2], case.expected[2])
  assert np.array_equal(np.sort(wrong[1]), np.arange(case.n))     # still a permutation: only the ORDER is wrong


@pytest.mark.parametrize("n", [hb.N_PER9, hb.N_PER17, hb.N_PER1, hb.N_PER2])
def test_a_scan_without_the_partial_chunk_is_told_apart(n):
  case = CASES[f"scan_n{n}"]
  wrong = hb.route_by_tiles(case.ids, case.input_dim, case.rows_per_rank, case.world, drop_partial_chunk=True)
  assert not np.array_equal(wrong[1], case.expected[1])
  # ... and the shapes the suite had (per <= 2: a partial chunk only) never reach a FULL chunk followed by a partial one
  full_chunks = {hb.N_PER9: 1, hb.N_PER17: 2, hb.N_PER1: 0, hb.N_PER2: 0}
  assert max(full for full, _ in _lanes(300_000)[2]) == 0 and max(full for full, _ in _lanes(n)[2]) == full_chunks[n]


def test_workspace_bytes():
  assert hb.workspace_bytes(0, 8) == 256 and hb.workspace_bytes(1, 1) == 12 + 256
  assert hb.workspace_bytes(hb.N_PER17, 8) == 1031 * 8 * 12 + 256


# ---- B. fused lookups ------------------------------------------------------------------------------------------
def test_cells_name_their_table_row_and_column_exactly():
  t = hb.make_table(255, 256, 256)
  assert t.dtype == np.float32 and t[255, 255] == 2 ** 24 - 1 and t[0, 0] == 255 * 65536
  cells = np.concatenate([hb.make_table(u, 256, 256).reshape(-1) for u in (0, 1, 3, 129, 255)])
  assert len(np.unique(cells)) == cells.size                      # a misplaced cell shows up as itself
  assert (cells == np.round(cells)).all() and cells.max() < 2 ** 24
  assert [hb.table_of(u) for u in range(7)] == [0, 1, 0, 3, 4, 3, 6]     # shared and own tables


def test_launches_and_out_chunk0():
  assert hb.lookup_launches(1, 16) == [(0, 1)] and hb.lookup_launches(16, 16) == [(0, 16)]
  assert hb.lookup_launches(17, 16) == [(0, 16), (16, 1)]
  assert hb.lookup_launches(33, 16) == [(0, 16), (16, 16), (32, 1)]
  assert [c0 for c0, _ in hb.lookup_launches(129, 64)] == [0, 64, 128]      # bucket_col0 of the multi kernel
  assert hb.lookup_launches(64, 64) == [(0, 64)] and hb.lookup_launches(65, 64) == [(0, 64), (64, 1)]


def test_per_row_of_every_dim():
  assert [d // 4 for d in hb.DIMS] == [1, 2, 4, 8, 16, 32, 64]
  for d in (12, 512):                                              # refused: not 4 * 2^k <= 256
    pr = d // 4
    assert pr > 64 or pr & (pr - 1)


def test_lookups_past_the_cap_and_live_lanes():
  total = hb.N_LOOKUP_PAST_CAP * 16
  assert total == 1_048_592 and hb.last_wave(total, hb.LOOKUP_CAP_BLOCKS) == (16, 16)
  assert total * 4 * 4 == 16_777_472                              # bytes of the D = 4 output
  assert hb.last_wave(hb.N_HASH_PAST_CAP, hb.HASH_CAP_BLOCKS) == (300, 300 % 64)
  assert hb.last_wave(900, hb.LOOKUP_CAP_BLOCKS) == (0, 4)
  for total, rem in ((64, 0), (65, 1), (127, 63), (63, 63), (129, 1), (192, 0)):
    assert total % 64 == rem


def test_a_lookup_that_ignores_out_chunk0_is_told_apart():
  for chunks in (17, 33):
    good = hb.unified_expected("i64", 5, chunks, 37, 4, -7.0)
    bad = hb.unified_expected("i64", 5, chunks, 37, 4, -7.0, ignore_chunk0=True)
    assert not np.array_equal(good[0], bad[0]) and not np.array_equal(good[1], bad[1])
    assert (good[0] != -7.0).all() and (bad[0][:, 16 * 4:] == -7.0).all()
  one = hb.unified_expected("i64", 5, 16, 37, 4, -7.0), hb.unified_expected("i64", 5, 16, 37, 4, -7.0, ignore_chunk0=True)
  assert np.array_equal(one[0][0], one[1][0])                     # a single launch cannot tell: hence 17 and 33


def test_unified_expected_against_the_oracle_directly():
  n, chunks, bins, d = 230, 4, 37, 8
  out, buckets = hb.unified_expected("i32", n, chunks, bins, d, -1.0)
  ids = hb.base_ids("i32")[np.arange(n) % hb.PERIOD]
  for c in range(chunks):
    want = o_hash.hash_bucket_strong(ids, bins, hb.salt_of(c))
    assert np.array_equal(buckets[:, c], want)
    table = hb.make_table(hb.table_of(c), bins, d)
    assert np.array_equal(out[:, c * d:(c + 1) * d], table[want])
  strings = hb.base_strings()
  out, buckets = hb.unified_expected("bytes", 30, 2, 256, 4, -1.0)
  assert buckets[:, 1].tolist() == [o_hash.siphash24(*hb.salt_of(1), s) % 256 for s in strings[:30]]
  assert n > hb.PERIOD and len(set(buckets[:, 1].tolist())) > 20


def test_multi_layout_and_expected():
  feature, chunk, declared = hb.multi_layout(5)
  assert (feature, chunk, declared) == ([0, 1, 1, 1, 2], [0, 0, 1, 2, 0], [1, 3, 2])       # the last feature is cut
  feature, chunk, declared = hb.multi_layout(129)
  assert len(feature) == 129 and all(c < declared[f] for f, c in zip(feature, chunk))
  last_of_feature = [u for u in range(129) if chunk[u] == declared[feature[u]] - 1]
  assert any(declared[feature[u]] > 1 for u in last_of_feature) and len(set(declared)) == 4
  assert feature[63] == feature[64] and feature[127] == feature[128]      # features that straddle two launches
  outs, b = hb.multi_expected("i64", 70, 5, 37, 4, -3.0)
  assert [o.shape for o in outs] == [(70, 4), (70, 12), (70, 8)] and b.shape == (70, 5)
  assert (outs[2][:, 4:] == -3.0).all() and (outs[2][:, :4] != -3.0).all()
  ids1 = hb.multi_ids("i64", 70, 1)
  assert np.array_equal(b[:, 2], o_hash.hash_bucket_strong(ids1, 37, hb.salt_of(2)))
  assert np.array_equal(outs[1][:, 4:8], hb.make_table(0, 37, 4)[b[:, 2]])      # unit 2 reads unit 0's table
  assert not np.array_equal(hb.multi_ids("i64", 70, 1), hb.multi_ids("i64", 70, 0))


# ---- C. hash kernels -------------------------------------------------------------------------------------------
def test_periodic_inputs():
  for kind, dtype in (("i32", np.int32), ("i64", np.int64)):
    ids = hb.base_ids(kind)
    assert ids.dtype == dtype and ids.size == hb.PERIOD == 211 and len(set(ids.tolist())) > 200
    assert {int(np.iinfo(dtype).min), int(np.iinfo(dtype).max), 0, -1} <= set(ids.tolist())
  strings = hb.base_strings()
  assert len(strings) == hb.PERIOD and [len(s) for s in strings[:41]] == list(range(41))
  assert any(b >= 0x80 for s in strings for b in s)
  blob, offsets = hb.pack_periodic(strings, 500)
  for i in (0, 1, 8, 210, 211, 212, 499):
    assert bytes(blob[offsets[i]:offsets[i + 1]]) == strings[i % hb.PERIOD]
  assert offsets[0] == 0 and offsets[-1] == blob.size


def test_a_hash_that_stops_at_the_grid_cap_is_told_apart():
  n, cap = hb.N_HASH_PAST_CAP, hb.HASH_CAP_BLOCKS * hb.BLOCK
  assert n - cap == 300
  for kind, bins in (("i32", 1009), ("i64", 1009), ("bytes", 1009), ("bytes", None)):
    good = hb.hash_expected(kind, n, bins, (3, 4))
    bad = hb.hash_expected(kind, n, bins, (3, 4), stop_at=cap, sentinel=-99)
    assert np.array_equal(good[:cap], bad[:cap]) and (good[cap:] != bad[cap:]).all()
  assert hb.hash_expected("bytes", 3, None, (3, 4))[1] == hb.as_signed(o_hash.siphash24(3, 4, hb.base_strings()[1]))


def test_barrett_by_hand_and_against_the_remainder():
  # m = 1: recip = 2^64 - 1, the estimate is h - 1, one subtraction brings 1 down to 0
  assert hb.barrett(12345, 1) == (0, 1, 1) and hb.barrett(0, 1) == (0, 0, 0)
  # m = 2^63 - 1: recip = 2, q = h >> 63; h = 2^64 - 1 = 2 m + 1 -> q = 1, r = 2^63, one subtraction -> 1
  assert hb.barrett(2 ** 64 - 1, 2 ** 63 - 1) == (1, 1, 1)
  # m = 3: recip = 0x5555...5, q = recip - 1 for h = 2^64 - 1 = 3 recip, r = 3, one subtraction -> 0
  assert hb.barrett(2 ** 64 - 1, 3) == (0, 1, 1)
  # m = 2^32: recip = 2^32 - 1; h = 2^64 - 1 -> q = 2^32 - 2, r = 2^33 - 1, one subtraction -> 2^32 - 1
  assert hb.barrett(2 ** 64 - 1, 2 ** 32) == (2 ** 32 - 1, 1, 1)
  rng = np.random.default_rng(0)
  hs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1] + [int(x) for x in
                                                                                     rng.integers(0, 2 ** 64, 500, dtype=np.uint64)]
  for m in hb.TOP_BINS + (1, 37, 256, 2 ** 62 + 7):
    for h in hs + [m - 1, m, m + 1, 2 * m - 1, (2 ** 64 // m) * m - 1, min((2 ** 64 // m) * m, 2 ** 64 - 1)]:
      r, _, deficit = hb.barrett(h, m)
      assert r == h % m and 0 <= deficit <= 2


# ---- D. row hash -----------------------------------------------------------------------------------------------
def test_mix64_and_both_row_hashes_by_hand():
  assert hb.mix64(0) == 0                                          # every step keeps 0
  # mix64(1): 1 -> x MIX1 = MIX1 -> ^ (MIX1 >> 33 = 0x7FA8D7EB) = 0xFF51AFD792FD5B26 -> x MIX2 -> ^ >> 33
  h = 0xFF51AFD7ED558CCD ^ 0x7FA8D7EB
  assert h == 0xFF51AFD792FD5B26
  h = h * 0xC4CEB9FE1A85EC53 % 2 ** 64
  assert hb.mix64(1) == h ^ (h >> 33) == 0xB456BCFC34C2CB2C        # MurmurHash3's fmix64(1)
  # the scalar chain on the one-word row [1.0f]: h0 = GOLD ^ d, one round
  h = 0x9E3779B97F4A7C15 ^ 1
  h ^= (0x3F800000 + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) % 2 ** 64
  h = h * 0xFF51AFD7ED558CCD % 2 ** 64
  h ^= h >> 33
  assert hb.row_hash_int([0x3F800000]) == h % 2 ** 63
  assert hb.row_hash_np(np.asarray([[1.0]], np.float32))[0] == h % 2 ** 63
  # one all-zero piece, d = 4: a = b = 0 under the key of piece 0 (k = GOLD, k << 1 | 1 = 0x3C6EF372FE94F82B)
  assert (0x9E3779B97F4A7C15 << 1 | 1) % 2 ** 64 == 0x3C6EF372FE94F82B
  h = (hb.mix64(0x9E3779B97F4A7C15) + hb.mix64(0x3C6EF372FE94F82B)) % 2 ** 64
  assert hb.row_hash_int([0, 0, 0, 0]) == hb.mix64(h ^ 4) % 2 ** 63 == hb.row_hash_np(np.zeros((1, 4), np.float32))[0]
  # the position constant: the same piece in slot 0 and in slot 1 of a two-piece row hashes differently
  assert hb.row_hash_int([1, 2, 3, 4, 0, 0, 0, 0]) != hb.row_hash_int([0, 0, 0, 0, 1, 2, 3, 4])


def test_row_hash_dispatch_rule():
  want = {4: ("pieces", 1), 8: ("pieces", 2), 12: ("pieces", 2), 20: ("pieces", 4), 100: ("pieces", 16),
          128: ("pieces", 32), 256: ("pieces", 32), 7: ("scalar", 1), 1: ("scalar", 1)}
  assert {d: hb.row_hash_route(d) for d in hb.ROW_DIMS} == want
  assert hb.row_hash_route(64) == ("pieces", 16) and hb.row_hash_route(64, base_address=4) == ("scalar", 1)
  # 12, 20 and 100 are piece counts (3, 5, 25) that are no power of two; 256 has more pieces (64) than lanes (32)
  assert [d // 4 for d in (12, 20, 100, 256)] == [3, 5, 25, 64]
  # reached through BruteForce.index before: d = 8, 16, 32, 64 only
  assert [hb.row_hash_route(d)[1] for d in (8, 16, 32, 64)] == [2, 4, 8, 16]
  for lpr in (1, 2, 4, 8, 16, 32):
    assert hb.ROW_N * lpr % 64 != 0 and hb.ROW_N * lpr > 256       # a partly empty last wave, more than one block


@pytest.mark.parametrize("d", hb.ROW_DIMS + (64,))
def test_row_hash_restatements_agree_and_tell_the_pairs_apart(d):
  c = hb.row_corpus(d)
  words = c.view(np.uint32)
  h = hb.row_hash_np(c)
  assert h.dtype == np.int64 and (h >= 0).all()
  for r in list(hb.PLANTED) + [2, 3, 4, 5, 6, 7, 100]:
    assert hb.row_hash_int(words[r].tolist()) == h[r]              # lane by lane in Python ints == NumPy
  assert len({int(h[r]) for r in hb.PLANTED}) == 1 and (words[list(hb.PLANTED)] == words[0]).all()
  for a, b in hb.PAIRS.values():
    assert (words[a] != words[b]).sum() == 1 and h[a] != h[b]
  a, b = hb.PAIRS["signed_zero"]
  assert c[a, d // 2] == c[b, d // 2] and words[a, d // 2] == 0 and words[b, d // 2] == 0x80000000
  assert (words[hb.PAIRS["last_word"][0]] != words[hb.PAIRS["last_word"][1]]).nonzero()[0].tolist() == [d - 1]
  assert (words[hb.PAIRS["first_word"][0]] != words[hb.PAIRS["first_word"][1]]).nonzero()[0].tolist() == [0]
  assert len(np.unique(h)) == len(np.unique(words, axis=0))        # no collision on this corpus
  if d % 4 == 0:                                                     # the scalar chain is another function
    hs = hb.row_hash_np(c, scalar=True)
    assert (hs != h).any() and hb.row_hash_int(words[9].tolist(), lanes=("scalar", 1)) == hs[9]
    # the sum over lanes wraps and commutes: any lane count gives the same value
    assert len({hb.row_hash_int(words[9].tolist(), lanes=("pieces", l)) for l in (1, 2, 4, 8, 16, 32)}) == 1


def test_dedup_corpora_hold_planted_copies():
  for d in hb.DEDUP_DIMS:
    c, q = hb.dedup_corpus(d)
    distinct = len(np.unique(c, axis=0))
    assert c.shape == (600, d) and q.shape == (9, d) and 440 <= distinct <= 450
    assert len(np.unique(hb.row_hash_np(c))) == distinct
  assert set(hb.DEDUP_DIMS).isdisjoint({8, 16, 32, 64})
