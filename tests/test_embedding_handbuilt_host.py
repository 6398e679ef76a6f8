"""The hand-built id lists of tests/embedding_handbuilt.py without a GPU: every property a builder claims to plant is
asserted again from the ids alone, the sort's plan of every vocabulary the GPU tests use is asked from the library
(``tfrs_embedding_sort_plan``, the function the sort itself calls), and the gradient rows make the order of summation
visible in the bits -- so tests/test_embedding_layout_gpu.py fails on a kernel that sums in another order."""

import ctypes

import numpy as np
import pytest

from tests import clippy_restatement as crs
from tests import embedding_handbuilt as hb
from tests import table_optimizers_restatement as rs

PIECES = (32, 64, 128, 256)       # piece_length(d) of the run-layout dims
RUN_DIMS = hb.RUN_DIMS


def test_piece_lengths_of_the_run_layout_dims():
  assert tuple(rs.piece_length(d) for d in RUN_DIMS) == (32, 32, 64, 64, 32, 128, 256)
  assert sorted({rs.piece_length(d) for d in RUN_DIMS}) == list(PIECES)
  # d == piece at 32, 64 and 128: the partial sums fill the sort's spare key buffer to its last float
  assert [d for d in RUN_DIMS if d == rs.piece_length(d)] == [32, 64, 128]


# ---- the sort's plan ----------------------------------------------------------------------------------------------------
def _plan(vocab):
  from recommenders_amd import _lib
  passes, digit_bits = ctypes.c_int(-1), ctypes.c_int(-1)
  _lib.check(_lib.load().tfrs_embedding_sort_plan(vocab, ctypes.byref(passes), ctypes.byref(digit_bits)))
  return passes.value, digit_bits.value


def test_sort_plan_of_every_vocabulary_in_the_table():
  for vocab, plan in hb.SORT_PLANS.items():
    assert _plan(vocab) == plan, vocab
  # every sort_*_kernel<BITS> instantiation at one, two and three passes
  assert {plan for plan in hb.SORT_PLANS.values()} == {(p, b) for p in (1, 2, 3) for b in (8, 9, 10)}
  assert _plan(2 ** 30) == (4, 8) and _plan(2 ** 32 - 2) == (4, 8)       # (left to the large tests)
  assert _plan(1) == (1, 8)


def test_sort_plan_covers_the_bits_of_the_vocabulary_and_the_invalid_key():
  """With 2^bits > vocab the plan covers bits + 1 bits (bit `bits` is set in the invalid key 0xFFFFFFFF and in no valid
  one, so it sorts last) in the fewest passes of 8, 9 or 10 bits, at the narrowest digit that needs no more passes; never
  more than 4 x 8 = the 32 bits of a key."""
  for vocab in sorted(set(hb.SORT_PLANS) | {1, 2, 3, 2 ** 16, 2 ** 26, 2 ** 30 - 1, 2 ** 30, 2 ** 32 - 2}):
    passes, digit_bits = _plan(vocab)
    need = int(vocab).bit_length() + 1
    fewest = min(4, min(-(-need // b) for b in (8, 9, 10)))
    assert passes == fewest, vocab
    assert digit_bits == min(b for b in (8, 9, 10) if min(4, -(-need // b)) == fewest), vocab
    assert passes * digit_bits >= min(need, 32), vocab


def test_sort_plan_rejects_bad_arguments():
  from recommenders_amd import _lib
  a, b = ctypes.c_int(), ctypes.c_int()
  assert _lib.load().tfrs_embedding_sort_plan(0, ctypes.byref(a), ctypes.byref(b)) == _lib.TFRS_EINVAL
  assert _lib.load().tfrs_embedding_sort_plan(5, None, ctypes.byref(b)) == _lib.TFRS_EINVAL


@pytest.mark.parametrize("vocab", sorted(hb.SORT_PLANS))
def test_sort_plan_ids_reach_both_ends_of_the_key(vocab):
  passes, digit_bits = hb.SORT_PLANS[vocab]
  mask = (1 << digit_bits) - 1
  top_shift = digit_bits * (passes - 1)
  for n in hb.SORT_NS:
    ids, pool = hb.sort_plan_ids(vocab, n, passes, digit_bits)
    assert ids.size == n and ids.dtype == np.int64
    valid = ids[(ids >= 0) & (ids < vocab)]
    if n == 1:
      assert ids.tolist() == [vocab - 1]
      continue
    assert (ids == -1).any() and (ids == vocab).any()
    have = set(valid.tolist())
    assert {0, vocab - 1} <= have
    # two ids that differ in the bottom digit only, two that differ in the top digit only (one pass: the same digit)
    assert {0, 1, 2, 3} <= have
    pairs = [(x, y) for x in pool for y in pool if x < y and (x ^ y) >> top_shift and not (x ^ y) & ((1 << top_shift) - 1)]
    assert pairs and all(x in have and y in have for x, y in pairs)
    assert (valid >> top_shift).max() == (vocab - 1) >> top_shift        # keys in the top digit's last used bucket
    assert ((valid & mask) == mask).any() or vocab <= mask                # ... and in the bottom digit's last bucket
    # duplicates whose order is visible: runs with continuing pieces at the piece of d = 4
    _, start, length, nvalid = hb.runs_of(ids, vocab)
    assert (hb.continuing_pieces(start, length, 32) >= 3).any()
    assert nvalid < n
  tiles = -(-hb.SORT_NS[-1] // hb.SORT_TILE)
  assert 4 * tiles > hb.SORT_SCAN_CHUNK and hb.SORT_NS[-1] % hb.SORT_TILE        # two scan chunks, a partial tile
  assert 4095 % hb.SORT_TILE and 4097 > hb.SORT_TILE                              # one partial tile; a tile and one key


def test_sort_plan_rows_show_the_order():
  vocab = 512
  ids, _ = hb.sort_plan_ids(vocab, 4097, *hb.SORT_PLANS[vocab])
  rows = hb.gradient_rows(np.random.default_rng(4097), ids.size, 4)
  differs, short, reversed_differs = hb.order_is_visible(ids, rows, vocab, 32)
  assert differs.size >= 1 and short >= 2 and 2 * reversed_differs >= short


# ---- run layouts --------------------------------------------------------------------------------------------------------
def _runs(case):
  run_id, start, length, nvalid = hb.runs_of(case["ids"], case["vocab"])
  return run_id, start, length, nvalid, hb.continuing_pieces(start, length, case["piece"])


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("variant", ["invalid", "end_aligned", "end_ragged"])
def test_run_layout_holds_every_planted_run(variant, piece, id_dtype):
  case = hb.run_layout_case(piece, variant, id_dtype)
  ids, vocab, n, p = case["ids"], case["vocab"], case["n"], piece
  assert ids.dtype == id_dtype and ids.size == n
  run_id, start, length, nvalid, cont = _runs(case)
  end = start + length
  cut = hb.first_cut(start, p)

  def some(mask):
    assert mask.any()
    return mask

  some(length == 1)
  some((start % p == 0) & (length == p))                             # ends exactly at its first cut, no continuation
  assert (cont[(start % p == 0) & (length == p)] == 0).all()
  some((start % p == 1) & (length == p - 1))                         # p - 1 from 1: ends at a multiple that is no cut
  some((start % p == 0) & (length == p + 1) & (cont == 1))           # a continuing piece of one element
  ragged = some((start % p != 0) & (cont >= 2) & ((cut - start) % p != 0) & ((end - cut) % p != 0) & ((end - cut) % p < p // 2))
  some(cont >= 3)
  long_run = cont >= 1
  some(long_run[1:] & long_run[:-1])                                 # a long run directly behind another long run
  assert long_run[-1] and end[-1] == nvalid                          # the last run is long and ends the valid keys
  if variant == "invalid":
    assert nvalid < n                                                # ... directly followed by the invalid keys
    invalid = ids.astype(np.int64)[(ids < 0) | (ids.astype(np.int64) >= vocab)]
    want = {-1, vocab, hb.INT32_MAX} | ({hb.WRAPS_TO_3} if id_dtype == np.int64 else set())
    assert set(invalid.tolist()) == want
    where = np.flatnonzero((ids < 0) | (ids.astype(np.int64) >= vocab))
    assert where.min() == 0 and where.max() > n // 2 and np.diff(where).min() > 1      # scattered, not a block
  else:
    assert nvalid == n and end[-1] == n                              # the run reaches n
    assert n % p == (0 if variant == "end_aligned" else 5)
  assert {0, 3, vocab - 1} <= set(run_id.tolist())                   # 2^32 + 3 would land on a touched row
  assert ragged.sum() >= 1
  # the occurrence order is not the sorted order
  valid = ids[(ids >= 0) & (ids.astype(np.int64) < vocab)]
  assert (np.diff(valid.astype(np.int64)) < 0).sum() > valid.size // 4
  assert case["zero_pair"] in run_id.tolist() and length[run_id == case["zero_pair"]] == 2


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("piece", PIECES)
def test_degenerate_and_short_run_layouts(piece, id_dtype):
  case = hb.run_layout_case(piece, "short", id_dtype)
  run_id, start, length, nvalid, cont = _runs(case)
  assert length.max() == piece - 1 and (cont == 0).all() and nvalid < case["n"]
  assert ((start % piece == 1) & (length == piece - 1)).any() and (length == 1).any()
  assert {0, 3, case["vocab"] - 1} <= set(run_id.tolist())
  case = hb.run_layout_case(piece, "all_equal", id_dtype)
  run_id, start, length, nvalid, cont = _runs(case)
  assert run_id.tolist() == [3] and length.tolist() == [case["n"]] and nvalid == case["n"] and cont[0] == 3
  assert case["n"] % piece == 5
  case = hb.run_layout_case(piece, "all_invalid", id_dtype)
  assert hb.runs_of(case["ids"], case["vocab"])[3] == 0 and case["n"] == 100


@pytest.mark.parametrize("d", RUN_DIMS)
@pytest.mark.parametrize("variant", ["invalid", "end_aligned", "end_ragged", "short", "all_equal"])
def test_run_layout_rows_show_the_order_of_summation(variant, d):
  """For at least one long run the piece-order sum differs in bits from the single chain (every long run, in fact, is
  required to unless the case has several); reversing the occurrence order changes the bits of at least half of the
  short runs, so an unstable sort shows; the cancelling pair sums to exactly +0 and some rows hold -0.0."""
  piece = rs.piece_length(d)
  case = hb.run_layout_case(piece, variant)
  rows = hb.run_layout_rows(case, d)
  assert rows.dtype == np.float32 and rows.shape == (case["n"], d)
  assert (hb.bits(rows) == 0x80000000).any()
  mag = np.abs(rows[rows != 0])
  assert mag.max() / mag.min() > 1e6                                 # the deliberately mixed scale
  differs, short, reversed_differs = hb.order_is_visible(case["ids"], rows, case["vocab"], piece)
  if variant != "short":
    assert differs.size >= 1
  if variant != "all_equal":
    assert short >= len(hb.SHORT_RUNS) and 2 * reversed_differs >= short
    uniq, g = crs.sum_duplicates(case["ids"], rows, case["vocab"])
    assert (hb.bits(g[uniq == case["zero_pair"]]) == 0).all()        # exactly +0
    assert (g[uniq != case["zero_pair"]] != 0).any(axis=1).all()


# ---- the row scan's chunks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("vocab", hb.CHUNK_VOCABS)
@pytest.mark.parametrize("n", hb.CHUNK_NS)
def test_chunk_case_holds_what_it_names(n, vocab, id_dtype):
  case = hb.chunk_case(n, vocab, id_dtype)
  ids, planted = case["ids"], case["planted"]
  assert ids.dtype == id_dtype and ids.size == n
  wide = ids.astype(np.int64)
  assert wide[n - 1] == planted["last"] == vocab - 1                 # an id at the very last position
  if n > 7:
    assert ((wide < 0) | (wide >= vocab)).any()
  assert ("hot" in planted) == (n >= 4095) and ("straddle" in planted) == (n >= 4097)
  if "hot" in planted:
    pos = np.flatnonzero(wide[:hb.ROWSCAN_CHUNK] == planted["hot"])
    assert pos.size >= hb.ROWSCAN_HIT_CAP + 2                        # >= 130 inside the first chunk: a flush
    per_step = np.bincount(pos // 64, minlength=64)
    assert per_step[2] == 64                                         # all 64 lanes of one aligned step hit
    # the flush fires where the kernel tests it: walking the steps that hold a hit, nh + 64 exceeds the cap
    nh, flushed = 0, 0
    for c in per_step[per_step > 0]:
      if nh + 64 > hb.ROWSCAN_HIT_CAP:
        nh, flushed = 0, flushed + 1
      nh += c
    assert flushed >= 1
  if "straddle" in planted:
    assert wide[hb.ROWSCAN_CHUNK - 1] == wide[hb.ROWSCAN_CHUNK] == planted["straddle"]
  assert set(hb.CHUNK_VOCABS) >= {1, 2, 5, 7} and any(v % 4 == 0 for v in hb.CHUNK_VOCABS)
  assert [m % hb.ROWSCAN_CHUNK for m in hb.CHUNK_NS] == [1, 4095, 0, 1, 1] and max(hb.CHUNK_NS) > 2 * hb.ROWSCAN_CHUNK


def test_chunk_case_rows_show_the_order():
  case = hb.chunk_case(8193, 7)
  rows = hb.gradient_rows(np.random.default_rng(1), 8193, 3)
  _, chain = crs.sum_duplicates(case["ids"], rows, 7)
  _, rev = crs.sum_duplicates(case["ids"][::-1], rows[::-1], 7)
  assert (hb.bits(chain) != hb.bits(rev)).any(axis=1).sum() >= 4


# ---- the combiner's bags ------------------------------------------------------------------------------------------------
def test_bag_cases_hold_every_length_and_every_empty_position():
  u = hb.SEGMENT_ROUND
  a = hb.bag_case("empty_last", 50)
  lens = a["lengths"]
  assert set(lens.tolist()) == set(hb.BAG_LENGTHS)
  assert lens[0] == 0 and lens[-1] == 0                              # empty first and last
  assert ((lens[1:] == 0) & (lens[:-1] == 0)).sum() >= 2             # ... and in pairs
  assert np.array_equal(np.diff(a["row_splits"]), lens) and a["row_splits"][0] == 0
  assert a["ids"].size == a["row_splits"][-1] and a["ids"].min() >= 0 and a["ids"].max() < 50
  # a first round that is partly clamped (1, 7), exactly full (8, 16), a second round of one entry (9, 17), five rounds
  assert {1, 7} <= set(lens.tolist()) and {u, 2 * u} <= set(lens.tolist()) and {u + 1, 2 * u + 1} <= set(lens.tolist())
  assert 40 // u == 5 and 40 in lens
  b = hb.bag_case("full_last", 50)
  assert set(b["lengths"].tolist()) == set(hb.BAG_LENGTHS)
  assert b["row_splits"][-1] == b["ids"].size and b["lengths"][-1] % u != 0 and b["lengths"][-1] > u
  c = hb.bag_case("all_empty", 50)
  assert c["ids"].size == 0 and (c["row_splits"] == 0).all() and c["lengths"].size == 5


def test_bag_weights_make_every_product_exact_or_not():
  case = hb.bag_case("empty_last", 50)
  w = hb.bag_weights(case, "pow2")
  assert w.dtype == np.float32 and set(w.tolist()) == {0.5, 1.0, 2.0, 4.0}
  table = hb.gradient_rows(np.random.default_rng(3), 50, 5)
  prod = w[:, None].astype(np.float64) * table[case["ids"]].astype(np.float64)
  assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)          # exact in float32
  w2 = hb.bag_weights(case, "any")
  prod2 = w2[:, None].astype(np.float64) * table[case["ids"]].astype(np.float64)
  assert not np.array_equal(prod2.astype(np.float32).astype(np.float64), prod2)
