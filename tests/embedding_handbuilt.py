"""Hand-built id lists for the embedding kernels (csrc/embedding.hip, csrc/sparse_update.hip): every builder returns the ids together with a
description of the structure it planted, so a test chooses the layout the kernels see -- run starts and lengths against
the piece cuts of the sorted route, occurrences against the LDS chunks and the hit list of the row scan, bag lengths
against the rounds of the combiner -- instead of taking what a random draw produces.  tests/test_embedding_handbuilt_host.py
proves every planted property again from the ids alone.  Pure numpy, no GPU access.  Test infrastructure only."""

import numpy as np

from tests import clippy_restatement as crs
from tests import table_optimizers_restatement as rs

ROWSCAN_CHUNK = 4096      # kRowscanChunk: ids per LDS chunk of the row scan
ROWSCAN_HIT_CAP = 128     # kRowscanHitCap: hits a wave records before it has to flush
SEGMENT_ROUND = 8         # kU: entries per round of the combiner forward
INT32_MAX = 2 ** 31 - 1
WRAPS_TO_3 = 2 ** 32 + 3  # an int64 id that a truncation to 32 bits would turn into the valid id 3


def bits(a):
  """The float32 array's bit patterns (a comparison that sets -0 apart from +0)."""
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gradient_rows(rng, n, d, negative_zeros=True):
  """[n, d] float32 of deliberately mixed scale, normal * 10^uniform(-3, 3) per entry: the sum of a few of them depends
  on the order in the last bits.  Every 37th entry (flat) is -0.0."""
  g = (rng.normal(size=(n, d)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(n, d))).astype(np.float32)
  if negative_zeros:
    g.reshape(-1)[5::37] = -0.0
  return g


def runs_of(ids, vocab):
  """(id, start, length) of every run of the stably sorted valid ids -- the list the sorted route's scatter sees before
  the invalid keys -- as three int64 arrays, and the number of valid ids."""
  ids = np.asarray(ids).reshape(-1).astype(np.int64)
  valid = np.sort(ids[(ids >= 0) & (ids < vocab)], kind="stable")
  if not valid.size:
    z = np.zeros((0,), np.int64)
    return z, z, z, 0
  start = np.flatnonzero(np.r_[True, valid[1:] != valid[:-1]])
  length = np.diff(np.r_[start, valid.size])
  return valid[start], start.astype(np.int64), length.astype(np.int64), int(valid.size)


def first_cut(start, piece):
  """Where the sorted route cuts a run that starts at ``start`` for the first time (``first_end`` of
  scatter_add_u32_kernel): the first multiple of ``piece`` at least ``piece`` positions into the run."""
  return ((np.asarray(start) + piece - 1) // piece + 1) * piece


def continuing_pieces(start, length, piece):
  """Number of pieces after the first one (the partial sums scatter_add_pieces_kernel writes for the run)."""
  rest = np.asarray(start) + np.asarray(length) - first_cut(start, piece)
  return np.where(rest > 0, (rest + piece - 1) // piece, 0)


def invalid_ids(vocab, id_dtype):
  """The invalid ids a list mixes in: -1, vocab, INT32_MAX and -- int64 lists only -- 2^32 + 3."""
  out = [-1, vocab, INT32_MAX]
  if np.dtype(id_dtype) == np.int64:
    out.append(WRAPS_TO_3)
  return out


def _spread(valid_sorted, invalid, seed, id_dtype):
  """The sorted valid ids spread into an occurrence order by a fixed permutation, the invalid ones inserted at evenly
  scattered positions."""
  rng = np.random.default_rng(seed)
  occ = np.asarray(valid_sorted, np.int64)[rng.permutation(len(valid_sorted))]
  if len(invalid):
    where = np.linspace(0, occ.size, num=len(invalid), endpoint=False).astype(np.int64)
    occ = np.insert(occ, where, np.asarray(invalid, np.int64))
  return occ.astype(id_dtype)


RUN_DIMS = (8, 32, 36, 64, 7, 128, 132)           # widths of the run-layout case: pieces of 32, 32, 64, 64, 32, 128, 256
ROWSCAN_DIMS = (1, 63, 64, 65, 128, 129, 256)     # widths of the chunk case: NS = 1, 2 and 4 at both ends
COMBINER_DIMS = (4, 12, 7, 32, 260)               # widths of the bag case
RUN_VARIANTS = ("invalid", "end_aligned", "end_ragged", "short", "all_equal", "all_invalid")
SHORT_RUNS = (3, 4, 5, 6, 7, 3, 5, 7, 4, 6, 3, 7)


def run_layout_case(piece, variant, id_dtype=np.int64, seed=0):
  """One id list for the sorted route at piece length ``piece`` (a power of two >= 32).

  The list is given as counts per ascending id and then spread into an occurrence order (``_spread``).  With i a run's
  start in sorted order the full variants hold, in this order: a run of ``piece`` from 0 (it ends exactly at its first
  cut); a run of 1; a run of ``piece - 1`` from ``piece + 1`` (i % piece == 1: it ends at a multiple of ``piece`` that is
  not a cut of its own); a run of ``piece + 1`` from an aligned start (one continuing piece of one element); a run from
  a misaligned start with a ragged first piece of 2 piece - 1, one whole piece and a last piece of 3 (a first piece
  SHORTER than ``piece`` does not exist on this route: ``first_cut`` is at least ``piece`` positions into the run, so
  a first piece holds piece .. 2 piece - 1 positions; the ragged one is the longest of them); directly behind it a run with
  three continuing pieces; the ``SHORT_RUNS`` (3 .. 7 occurrences); a run of 2 whose rows cancel (``zero_pair``: the
  test plants x, -x there); a run of 1 and the last, long run (two continuing pieces), which

    ``invalid``      is directly followed by the invalid keys (-1, vocab, INT32_MAX, 2^32 + 3 at scattered positions);
    ``end_aligned``  reaches n, n % piece == 0 (no invalid ids: the sorted list ends with the run);
    ``end_ragged``   reaches n, n % piece == 5.

  ``short``: only the runs shorter than ``piece`` (the row scan and the sorted route must agree on it), with invalid
  ids.  ``all_equal``: one run of n = 3 piece + 5.  ``all_invalid``: 100 invalid ids and nothing else.
  Id 3 is always a touched row where any is, id 0 and id vocab - 1 too.  Returns a dict: ids, vocab, n, piece, variant,
  zero_pair (the id of the cancelling run, or None)."""
  assert variant in RUN_VARIANTS and piece >= 32 and piece & (piece - 1) == 0
  p = piece
  vocab = 61
  inv = invalid_ids(vocab, id_dtype)
  zero_pair = None
  if variant == "all_equal":
    counts, invalid = {3: 3 * p + 5}, []
  elif variant == "all_invalid":
    counts, invalid = {}, (inv * 34)[:100]
  else:
    lengths = []
    if variant != "short":
      lengths += [p]                      # ends exactly at its first cut
    lengths += [1]
    if variant == "short":
      lengths += [p - 1]                  # from 1
    else:
      lengths += [p - 1, p + 1, (2 * p - 1) + p + 3, (2 * p - 3) + 2 * p + 5]
    lengths += list(SHORT_RUNS) + [2, 1]
    zero_at = len(lengths) - 2
    if variant != "short":
      at = sum(lengths)
      last = first_cut(at, p) - at + p + 7          # first piece, one whole piece, a last piece of 7
      if variant == "end_aligned":
        last += -(at + last) % p
      elif variant == "end_ragged":
        last += (5 - (at + last)) % p
      lengths += [int(last)]
    # ascending ids: 0, 3 and vocab - 1 among them
    ids_of = [0, 3] + list(range(5, 5 + 2 * (len(lengths) - 3), 2)) + [vocab - 1]
    assert len(ids_of) == len(lengths) and ids_of[-2] < vocab - 1
    counts = dict(zip(ids_of, lengths))
    zero_pair = ids_of[zero_at]
    invalid = [] if variant in ("end_aligned", "end_ragged") else (inv * 3)[:9]
  valid_sorted = np.repeat(np.fromiter(counts.keys(), np.int64, len(counts)),
                           np.fromiter(counts.values(), np.int64, len(counts)))
  ids = _spread(valid_sorted, invalid, seed + 17 * p, id_dtype)
  return dict(ids=ids, vocab=vocab, n=int(ids.size), piece=p, variant=variant, zero_pair=zero_pair)


def run_layout_rows(case, d, seed=0):
  """Gradient rows for ``case`` at width ``d``; the two occurrences of ``zero_pair`` get x and -x (their sum is +0)."""
  rng = np.random.default_rng(1000 * seed + 31 * case["piece"] + d + RUN_VARIANTS.index(case["variant"]))
  rows = gradient_rows(rng, case["n"], d)
  if case["zero_pair"] is not None:
    a, b = np.flatnonzero(case["ids"].astype(np.int64) == case["zero_pair"])
    rows[b] = -rows[a]
  return rows


CHUNK_NS = (1, 4095, 4096, 4097, 8193)
CHUNK_VOCABS = (1, 2, 5, 7, 8)


def chunk_case(n, vocab, id_dtype=np.int64, seed=0):
  """One id list for the row scan: random valid ids with an invalid one at every 53rd position, and planted, as far as
  ``n`` and ``vocab`` leave room (``planted`` names what is there):

    ``hot``       id ``hot`` at all 64 positions of the aligned step [128, 192) and at 72 further positions of the first
                  chunk, three per 64-position step from 256 on: at least 136 hits inside one chunk, more than the hit
                  cap (n >= 4095);
    ``straddle``  id vocab - 1 at positions 4095 and 4096, one each side of the chunk boundary (n >= 4097);
    ``last``      the last position holds the valid id vocab - 1 (always).

  With vocab = 1 every valid id is 0 and it is hot and straddles by itself.  Returns a dict: ids, vocab, n, planted."""
  rng = np.random.default_rng(seed + 7919 * vocab + n)
  ids = rng.integers(0, vocab, size=n).astype(np.int64)
  inv = invalid_ids(vocab, id_dtype)
  for k, pos in enumerate(range(7, n, 53)):
    ids[pos] = inv[k % len(inv)]
  planted = {}
  hot = 0 if vocab < 3 else 2
  if n >= 4095:
    ids[128:192] = hot
    ids[256 + 64 * np.arange(24)[:, None] + np.array([1, 30, 63])[None, :]] = hot   # 72 more, steps 4 .. 27
    planted["hot"] = hot
  if n >= 4097:
    ids[4095:4097] = vocab - 1
    planted["straddle"] = vocab - 1
  ids[n - 1] = vocab - 1
  planted["last"] = vocab - 1
  return dict(ids=ids.astype(id_dtype), vocab=vocab, n=n, planted=planted)


BAG_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 40)


def bag_case(kind, vocab, seed=0):
  """Row splits and ids for the combiner.  ``kind``:

    ``empty_last``  bags of 0, 0, 1, 7, 0, 8, 9, 0, 0, 16, 17, 40, 0 entries: every length of BAG_LENGTHS, empty bags
                    first, last and in pairs;
    ``full_last``   40, 0, 17, 16, 0, 0, 8, 7, 1, 9: the last bag ends on the last id of the list, in a partly clamped
                    second round;
    ``all_empty``   five empty bags and no id at all.

  The ids are random valid ones.  Returns a dict: ids, row_splits (both int64), lengths, vocab."""
  lengths = dict(empty_last=[0, 0, 1, 7, 0, 8, 9, 0, 0, 16, 17, 40, 0], full_last=[40, 0, 17, 16, 0, 0, 8, 7, 1, 9],
                 all_empty=[0] * 5)[kind]
  rng = np.random.default_rng(seed + len(lengths))
  splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
  ids = rng.integers(0, vocab, size=int(splits[-1])).astype(np.int64)
  return dict(ids=ids, row_splits=splits, lengths=np.asarray(lengths, np.int64), vocab=vocab, kind=kind)


def bag_weights(case, kind, seed=0):
  """``pow2``: drawn from {0.5, 1, 2, 4}, so every product w * e is exact; ``any``: uniform(0.25, 3)."""
  rng = np.random.default_rng(seed + 99)
  nnz = case["ids"].size
  if kind == "pow2":
    return rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=nnz)
  return rng.uniform(0.25, 3.0, size=nnz).astype(np.float32)


# vocabulary -> (passes, digit bits) of the radix sort, as tfrs_embedding_sort_plan answers (the host test asserts every
# entry through it): both ends of every plan below 2^30.  256 .. 511 is ONE pass of 10 bits (9 bits of ids and the bit
# that sets the invalid key apart), so two passes of 8 begin at 512.
SORT_PLANS = {100: (1, 8), 127: (1, 8), 128: (1, 9), 255: (1, 9), 256: (1, 10), 511: (1, 10), 512: (2, 8),
              32767: (2, 8), 32768: (2, 9), 131071: (2, 9), 131072: (2, 10), 524287: (2, 10), 524288: (3, 8),
              2 ** 23: (3, 9), 2 ** 27: (3, 10)}
SORT_NS = (1, 4095, 4097, 70001)      # the last: 18 tiles = 72 segments (two scan chunks) and a partial last tile
SORT_TILE = 4096
SORT_SCAN_CHUNK = 64


def sort_plan_ids(vocab, n, passes, digit_bits, seed=0):
  """``n`` ids for the radix sort of plan ``passes`` x ``digit_bits``: half of them from a small pool that holds 0 .. 3
  (they differ in the bottom digit only), vocab - 1, vocab - 2 and pairs x, x + 2^(top digit's shift) that differ in the
  top digit only -- long runs whose order shows in the sums --, half uniform over [0, vocab), and -1 / vocab at every
  97th position.  n == 1: the single id vocab - 1.  Returns (ids int64, pool)."""
  rng = np.random.default_rng(seed + vocab % 100003 + n)
  top = 1 << (digit_bits * (passes - 1))
  pool = [0, 1, 2, 3, vocab - 1, vocab - 2, (1 << digit_bits) - 1]      # (the last: the bottom digit's last bucket)
  for x in (0, 1, 5):
    pool += [x, x + top, vocab - 1 - x, vocab - 1 - x - top]
  pool = np.unique([x for x in pool if 0 <= x < vocab]).astype(np.int64)
  if n == 1:
    return np.array([vocab - 1], np.int64), pool
  ids = rng.integers(0, vocab, size=n).astype(np.int64)
  pick = rng.random(n) < 0.5
  ids[pick] = pool[rng.integers(0, pool.size, size=int(pick.sum()))]
  ids[:pool.size] = pool                       # every pool id at least once
  ids[pool.size::97] = -1
  ids[pool.size + 50::97] = vocab
  return ids, pool


def order_is_visible(ids, rows, vocab, piece):
  """What the host test asserts about a case's rows: (ids of the runs with a continuing piece whose piece-order sum
  differs in bits from the single chain, number of runs of 3 .. piece - 1 occurrences, number of those whose sum changes
  in bits when the occurrence order is reversed)."""
  uniq, chain = crs.sum_duplicates(ids, rows, vocab)
  uniq_p, pieces = rs.sum_duplicates(ids, rows, vocab, piece)
  assert np.array_equal(uniq, uniq_p)
  _, rev = crs.sum_duplicates(np.asarray(ids)[::-1], np.asarray(rows)[::-1], vocab)
  run_id, start, length, _ = runs_of(ids, vocab)
  assert np.array_equal(run_id, uniq)
  long_runs = continuing_pieces(start, length, piece) > 0
  differs = (bits(chain) != bits(pieces)).any(axis=1)
  assert not differs[~long_runs].any()         # a run without a continuing piece IS the single chain
  short = (length >= 3) & (length < piece)
  reversed_differs = (bits(chain) != bits(rev)).any(axis=1)
  return uniq[long_runs & differs], int(short.sum()), int((short & reversed_differs).sum())
