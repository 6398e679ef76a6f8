"""The hand-built lists of tests/select_handbuilt.py, proved on the host from the arrays alone: the restated order
against a brute-force Python sort, the restated dense walk and ``consume`` / ``absorb_chunk`` bookkeeping against the
expected lists, and for every case of tests/test_select_layout_gpu.py that it has the property it claims and reaches
the edge it is named for.  No GPU access.

What the bookkeeping model shows about the two monotone rows (the scalar walk offers the columns in order; the 16-byte
walk offers column 4 i + c of 64 pieces at a time, so a monotone row is not monotone in offer order there):
* descending, scalar walk: while fewer than k entries are held the bound is 0 and every offer passes, so the chunk
  fills once; the absorb this triggers is the only one before the end when nb > KP, the 64 keys that were compared
  against the stale bound ride into the chunk, and NOTHING passes afterwards.  The walk therefore absorbs exactly once
  (at the end) when nb <= KP and exactly twice (chunk full, end) otherwise.
* ascending, scalar walk: every offer passes at every point, one absorb per KP offered keys."""

import functools

import numpy as np
import pytest

from tests import select_handbuilt as hb


def _brute_force(scores, rows, k):
  """Top k by a Python sort with an explicit comparison; no numpy ordering."""
  def before(a, b):
    if a[0] != b[0]:                    # (-0.0 == 0.0 in Python as well)
      return -1 if a[0] > b[0] else 1
    return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)
  ent = sorted(((float(s), int(r)) for s, r in zip(scores, rows) if r >= 0), key=functools.cmp_to_key(before))[:k]
  out_s, out_r = np.zeros(k, np.float32), np.full(k, -1, np.int32)
  for i, (s, r) in enumerate(ent):
    out_s[i], out_r[i] = (0.0 if s == 0.0 else s), r
  return out_s.view(np.uint32), out_r


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_a_python_sort():
  rng = np.random.default_rng(1)
  alphabet = np.array([-0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, 2.5, 0.0, -0.0], np.float32)
  for n in (0, 1, 2, 7, 40):
    for k in (1, 3, 50):
      for _ in range(20):
        s = alphabet[rng.integers(0, alphabet.size, size=n)]
        r = rng.permutation(3 * n + 1)[:n].astype(np.int64) - 2           # some rows below 0
        r[rng.random(n) < 0.2] = -1
        got, want = hb.restated_topk(s, r, k), _brute_force(s, r, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (s, r, k)


def test_restatement_pins_the_zero_tie_the_empty_slots_and_the_top_row():
  s = np.array([-0.0, 0.0, -0.0, 1.0], np.float32)
  b, r = hb.restated_topk(s, [9, 4, 2, hb.TOP_ROW - 1], 6)
  assert r.tolist() == [hb.TOP_ROW - 1, 2, 4, 9, -1, -1]                  # the zeros tie: by row
  assert b.tolist() == [0x3F800000, 0, 0, 0, 0, 0]                        # -0.0 comes back as +0.0; empty = (0.0, -1)
  b, r = hb.restated_topk([5.0, 7.0], [-1, -5], 2)
  assert r.tolist() == [-1, -1] and b.tolist() == [0, 0]                  # rows below 0 do not exist


def test_keys_order_like_the_restatement():
  rng = np.random.default_rng(2)
  alphabet = np.array([-0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, 3.0e38, -1e-45], np.float32)
  s = alphabet[rng.integers(0, alphabet.size, size=300)]
  r = np.concatenate([rng.permutation(1000)[:298], [0, hb.TOP_ROW - 1]]).astype(np.int64)
  keys = hb.make_keys(s, r)
  assert keys.min() > 0                                                   # key 0 is free to mean "empty"
  got = hb.keys_to_lists(np.sort(keys)[::-1])
  want = hb.restated_topk(s, r, 300)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
  assert hb.keys_to_lists(np.zeros(2, np.uint64))[1].tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------ a. the dense walk
def _offer_keys(row, nb, aligned, base_row=0):
  out = []
  for cols in hb.dense_offers(nb, aligned):
    live = cols >= 0
    keys = np.zeros(64, np.uint64)
    keys[live] = hb.make_keys(row[cols[live]], base_row + cols[live])
    out.append(keys)
  return out


@pytest.mark.parametrize("nb", hb.DENSE_NB)
def test_both_walks_offer_every_column_exactly_once(nb):
  for aligned in (False, True):
    cols = np.concatenate(hb.dense_offers(nb, aligned))
    assert np.array_equal(np.sort(cols[cols >= 0]), np.arange(nb)), (nb, aligned)
  # lanes past the last whole piece offer nothing: with nb % 2048 != 0 the aligned walk has such lanes
  n4 = nb & ~3
  if n4 and n4 % 256:
    assert any((c < 0).any() for c in hb.dense_offers(nb, True)[:-1 if n4 < nb else None])


@pytest.mark.parametrize("nb", hb.DENSE_NB)
def test_planted_winners_sit_where_claimed(nb):
  pos, n4 = hb.planted_positions(nb), nb & ~3
  assert pos["tail"] == list(range(n4, nb)) and len(pos["tail"]) == nb % 4
  assert pos["last_piece"] == (list(range(n4 - 4, n4)) if n4 else [])
  for p in pos["batch_first"]:
    assert p % 2048 < 4
  for p in pos["batch_last"]:
    assert p % 2048 >= 2044 and p < n4
  assert len(pos["batch_first"]) == 4 * ((n4 + 2047) // 2048) and len(pos["batch_last"]) == 4 * (n4 // 2048)
  # in the walk: the first piece of a batch is lane 0 of its first offers, the last piece lane 63 of its last ones
  offers = hb.dense_offers(nb, True)
  for p in pos["batch_first"]:
    n, lane = next((n, int(np.flatnonzero(c == p)[0])) for n, c in enumerate(offers) if (c == p).any())
    assert lane == 0 and (n // 4) % 8 == 0
  for p in pos["batch_last"]:
    n, lane = next((n, int(np.flatnonzero(c == p)[0])) for n, c in enumerate(offers) if (c == p).any())
    assert lane == 63 and (n // 4) % 8 == 7
  # the planted row holds its distinct winners exactly there, above everything else
  row = hb.dense_row("planted", nb, 64, 0)
  at = hb.all_planted(nb)
  assert np.array_equal(np.flatnonzero(row >= 1000.0), at) and np.unique(row[at]).size == len(at)
  assert row[np.setdiff1d(np.arange(nb), at)].max(initial=-1.0) < 0


def test_patterns_are_what_they_are_named():
  for nb in hb.DENSE_NB:
    for k in (1, 65):
      for q in range(9):
        rows = {p: hb.dense_row(p, nb, k, q) for p in hb.PATTERNS}
        for v in rows.values():
          assert v.dtype == np.float32 and v.shape == (nb,) and not np.isnan(v).any()
        assert np.unique(rows["equal"]).size == 1
        assert (np.diff(rows["ascending"]) > 0).all() and (np.diff(rows["descending"]) < 0).all()
        if nb >= 2049:
          t = rows["tieblocks"]
          assert t[63] == t[64] and t[2047] == t[2048]                     # a block straddles an offer and a batch
          z = hb.bits(rows["zeros"])
          assert (z == 0).any() and (z == hb.NEG_ZERO).any()
          assert np.isneginf(rows["infs"]).any() and np.isposinf(rows["infs"]).sum() == (k >= 2)
  assert (hb.dense_row("ascending", 4099, 1, 0) == 0).any()                # the monotone rows pass through zero


@pytest.mark.parametrize("k", hb.KS)
def test_monotone_rows_absorb_as_claimed(k):
  kp = hb.kp_of(k)
  for nb in (65, 2049, 4099):
    want = hb.dense_case(5, nb, k)
    for q in range(5):
      pattern = hb.row_pattern(q)
      if pattern not in ("ascending", "descending"):
        continue
      row = want["scores"][q]
      for aligned in (False, True):
        best, log = hb.simulate(k, _offer_keys(row, nb, aligned))
        got = hb.keys_to_lists(best)
        assert np.array_equal(got[0], want["want_bits"][q]) and np.array_equal(got[1], want["want_rows"][q])
        mid = [a for a in log["absorbs"] if a[0] is not None]
        assert log["absorbs"][-1][0] is None                               # the walk ends with an absorb
        if pattern == "descending" and not aligned:
          assert len(mid) == (1 if nb > kp else 0)
          if mid:                                                          # ... and after it nothing passes
            assert mid[0][1] == kp and sum(log["passed"][mid[0][0] + 1:]) == 0
        if pattern == "ascending" and not aligned:
          assert all(p == 64 for p in log["passed"][:-1])                  # every offer passes
          assert len(mid) == (nb - 1) // kp
          if nb == 4099:
            assert len(mid) >= 2                                           # at least twice mid-stream at every KP
          if nb > kp:                                                      # fill + 64 == KP adds without an absorb,
            assert log["touch"] and all(t + 1 == m[0] for t, m in zip(log["touch"], mid))      # the next offer absorbs
        if pattern == "ascending" and aligned and nb == 4099:
          assert len(mid) >= 2


def test_partial_offers_reach_the_absorb_off_the_64_grid():
  """The tie-block and planted rows leave ``fill`` off the multiples of 64 when the absorb comes."""
  seen = set()
  for k in (63, 65, 129, 257):
    case = hb.dense_case(9, 2049, k)
    for q in range(9):
      for aligned in (False, True):
        best, log = hb.simulate(k, _offer_keys(case["scores"][q], 2049, aligned))
        got = hb.keys_to_lists(best)
        assert np.array_equal(got[0], case["want_bits"][q]) and np.array_equal(got[1], case["want_rows"][q])
        seen.update(f % 64 != 0 for n, f in log["absorbs"] if n is not None)
  assert seen == {False, True}


@pytest.mark.parametrize("nb", hb.DENSE_NB)
def test_alignment_cases_have_rows_on_both_walks(nb):
  layouts = hb.dense_layouts(nb)
  assert [ld - nb for ld, _ in layouts[:4]] == [0, 1, 2, 3]
  mixed = 0
  for ld, off in layouts:
    walks = {hb.row_is_aligned(r, ld, off) for r in range(9)}
    if ld % 4 == 0:
      assert walks == ({True} if off == 0 else {False})                    # all rows on one walk
    else:
      assert walks == {True, False}                                        # rows alternate inside one launch
      mixed += 1
  assert mixed >= 3 and layouts[-2][1] == 0 and layouts[-1][1] == 1


def _dense_cases():
  for nb in hb.DENSE_NB:
    for k in (1, 64, 65, 257):
      yield hb.dense_case(9, nb, k)
    yield hb.dense_case(9, nb, 65, base_row=hb.TOP_ROW - nb)
  for k in (1, 63, 65, 129, 1024):
    for nb in (1, 5, 70, 2052):
      for sl in sorted({0, 1, k - 1, k}):
        for base in (0, 5000, hb.TOP_ROW - nb):
          yield hb.dense_case(4, nb, k, state_len=sl, base_row=base)
      yield hb.dense_case(4, nb, k, state_len=k, base_row=5000, holes=True)


def test_dense_states_and_poison():
  short = ties = lower_wins = both_sides = 0
  for case in _dense_cases():
    nq, nb, k, sl, base = case["nq"], case["nb"], case["k"], case["state_len"], case["base_row"]
    assert np.isfinite(case["scores"]).all() or not np.isnan(case["scores"]).any()
    assert case["new_len"] == min(k, sl + nb)
    short += sl + nb < k
    for q in range(nq):
      ss, sr = case["state_real"][q]
      wb, wr = case["want_bits"][q], case["want_rows"][q]
      # the state is sorted, duplicate-free and disjoint from the block's rows
      assert np.array_equal(hb.restated_topk(ss, sr, sr.size)[1], sr)
      assert not ((sr >= base) & (sr < base + nb)).any()
      both_sides += bool((sr < base).any() and (sr >= base + nb).any())
      assert (wr >= 0).sum() == min(k, sr.size + nb)
      assert (wr[wr >= 0].size == np.unique(wr[wr >= 0]).size)
      if sl + nb < k:
        assert wr[-1] == -1 and wb[-1] == 0
      # ties between state and block on score, the lower row first -- from either side
      new_bits = hb.canonical_bits(case["scores"][q])
      common = np.intersect1d(hb.canonical_bits(ss), new_bits)
      ties += common.size > 0
      in_state = np.isin(wr, sr)
      for i in np.flatnonzero(wb[:-1] == wb[1:]):
        if wr[i + 1] >= 0 and in_state[i] != in_state[i + 1]:
          assert wr[i] < wr[i + 1]
          lower_wins += 1
      # every poison would enter the list if it were read: a column past nb, a state slot past state_len
      all_s = np.concatenate([ss, case["scores"][q]])
      all_r = np.concatenate([sr.astype(np.int64), base + np.arange(nb, dtype=np.int64)])
      for prow in (min(base + nb, hb.TOP_ROW - 1), hb.POISON_ROW):
        pb, pr = hb.restated_topk(np.append(all_s, case["poison"]), np.append(all_r, prow), k)
        assert not (np.array_equal(pb, wb) and np.array_equal(pr, wr)), (nb, k, sl, q)
      assert (case["state_bits"][q, sr.size:] == hb.INF_BITS).all()
      assert (case["state_rows"][q, sl:] == hb.POISON_ROW).all() and (case["state_rows"][q, sr.size:sl] == -1).all()
  assert short and ties and lower_wins and both_sides


def test_fold_cuts_cover_the_corpus():
  for cuts in hb.FOLD_CUTS:
    assert cuts[0] == 0 and cuts[-1] == hb.FOLD_NB and all(a < b for a, b in zip(cuts, cuts[1:]))
  assert [len(c) - 1 for c in hb.FOLD_CUTS] == [1, 2, 5]
  assert any(c % 4 for cuts in hb.FOLD_CUTS for c in cuts[1:-1])           # blocks start off the 16-byte grid too


# ------------------------------------------------------------------------------------------ b. parts
def test_merge_shapes_reach_the_edges_of_the_walk():
  ms = sorted({p * ki for p, ki in hb.MERGE_SHAPES})
  assert {p for p, _ in hb.MERGE_SHAPES} >= {1, 2, 8, 33} and {ki for _, ki in hb.MERGE_SHAPES} >= {1, 5, 100, 1024}
  for edge in (256, 512, 768):
    assert edge - 1 in ms and edge in ms and edge + 1 in ms                # m on both sides of 256 and of a multiple
  assert any(m % 64 for m in ms) and any(m % 256 == 0 for m in ms) and max(ms) == 33 * 1024
  for p, ki in hb.MERGE_SHAPES:
    ko = hb.merge_k_outs(p, ki)
    assert ko[0] == 1 and ko[-1] == min(p * ki, hb.MAX_K) and all(1 <= x <= min(p * ki, hb.MAX_K) for x in ko)
    if p * ki <= hb.MAX_K:
      assert p * ki in ko                                                  # k_out == nparts * k_in


@pytest.mark.parametrize("shape", hb.MERGE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_merge_cases_plant_what_they_say(shape):
  nparts, k_in = shape
  for nq in (1, 4, 5, 9):
    for few in (False, True):
      case = hb.merge_case(nparts, k_in, nq, few)
      s, r = case["scores"], case["rows"]
      assert not np.isnan(s).any() and np.isfinite(s[r >= 0]).all()
      assert (s[r < 0] == hb.INF).all()                                    # a slot that does not exist would win
      for q in range(nq):
        fr = case["flat_r"][q]
        assert np.unique(fr[fr >= 0]).size == (fr >= 0).sum()              # no row twice
        if case["empty_part"][q] >= 0:
          assert (r[case["empty_part"][q], q] == -1).all()
        if case["empty_part"][q] != nparts - 1 and not (few and q == 0):   # the clamped entry is the query's best
          assert r[nparts - 1, q, k_in - 1] >= 0 and s[nparts - 1, q, k_in - 1] == 9.0
          assert (s[:, q][r[:, q] >= 0] == 9.0).sum() == 1
        k_top = hb.merge_k_outs(nparts, k_in)[-1]
        wb, wr = hb.restated_topk(case["flat_s"][q], fr, k_top)
        pb, pr = hb.restated_topk(np.append(case["flat_s"][q], case["poison"]), np.append(fr, case["poison_row"]), k_top)
        assert not (np.array_equal(wb, pb) and np.array_equal(wr, pr))     # the poison of the gaps would enter
      if few:
        assert (case["flat_r"][0] < 0).all()                               # a query with nothing at all
        assert all((case["flat_r"][q] >= 0).sum() < max(hb.merge_k_outs(nparts, k_in)) or nparts * k_in < 40
                   for q in range(nq))
  if nparts >= 2 and k_in >= 100:
    case = hb.merge_case(nparts, k_in, 5)
    wb, wr = hb.merge_want(case, min(nparts * k_in, 129))
    tie_across = 0
    part_of = {}
    for p in range(nparts):
      for row in case["rows"][p, 0]:
        part_of[int(row)] = p
    for i in np.flatnonzero(wb[0][:-1] == wb[0][1:]):
      if wr[0][i + 1] >= 0:
        assert wr[0][i] < wr[0][i + 1]
        tie_across += part_of[int(wr[0][i])] != part_of[int(wr[0][i + 1])]
    assert tie_across                                                      # equal scores across parts, rows interleaved


# ------------------------------------------------------------------------------------------ c. expand
def _check_ranges(case):
  start, rows = case["dup_start"], case["dup_rows"]
  assert start[0] == 0 and start[-1] == rows.size and (np.diff(start) >= 1).all()
  assert np.array_equal(np.sort(rows), np.arange(rows.size))              # every original row in exactly one range
  canon = rows[start[:-1]]
  assert (np.diff(canon) > 0).all()                                        # distinct rows by ascending canonical row
  for u in range(start.size - 1):
    r = rows[start[u]:start[u + 1]]
    assert (np.diff(r) > 0).all() and r[0] == canon[u]                     # a range ascends from its canonical row
    assert (case["distinct_of_row"][r] == u).all()


def test_duplicate_ranges_are_built_as_the_layer_builds_them():
  groups = np.array([5, 9, 5, 2, 9, 9, 7, 2])                              # labels are arbitrary
  start, rows, of_row = hb.duplicate_ranges(groups)
  assert start.tolist() == [0, 2, 5, 7, 8] and rows.tolist() == [0, 2, 1, 4, 5, 3, 7, 6]
  assert of_row.tolist() == [0, 1, 0, 2, 1, 1, 3, 2]


@pytest.mark.parametrize("k_in", hb.EXPAND_K_IN)
def test_expand_cases_plant_what_they_say(k_in):
  for k_out in hb.EXPAND_K_OUT:
    for singles in (False, True):
      case = hb.expand_case(k_in, k_out, 5, singles)
      _check_ranges(case)
      s, u = case["scores"], case["distinct"]
      assert not np.isnan(s).any() and np.isfinite(s[u >= 0]).all() and (s[u < 0] == hb.INF).all()
      if singles:
        assert (case["mult"] == 1).all()
        continue
      assert {1, 2, 3, 63, 64, 65, k_out + 3} == set(case["mult"].tolist())
      listed = set()
      for q in range(5):
        v = np.flatnonzero(u[q] >= 0)
        assert np.array_equal(hb.restated_order(s[q][v], u[q][v]), np.arange(v.size))      # as a search returns them
        listed.update(case["mult"][u[q][v]].tolist())
        if k_in >= 64:
          per_group = [int((case["mult"][u[q][g:g + 64][u[q][g:g + 64] >= 0]] > 1).sum()) for g in range(0, k_in, 64)]
          assert per_group[0] >= 2 and (k_in < 130 or per_group[1] >= 2)   # several multi-row results in a group
      if k_in >= 64:
        assert listed >= {1, 2, 63, 64, 65, k_out + 3}
      assert (u < 0).any() and (hb.bits(s[u >= 0]) == hb.NEG_ZERO).any() == (k_in >= 64)
      wb, wr = hb.expand_want(case, k_out)
      for q in range(5):
        assert np.unique(wr[q][wr[q] >= 0]).size == (wr[q] >= 0).sum()
  assert (hb.expand_want(hb.expand_case(1, 1024, 5), 1024)[1][:, -1] == -1).all()      # fewer rows than k_out: empty slots


@pytest.mark.parametrize("k_out", hb.EXPAND_TIE_K)
def test_expand_tie_cases_really_tie(k_out):
  lists = {}
  for mode in ("tie", "lower", "short"):
    case = hb.expand_tie_case(k_out, mode)
    _check_ranges(case)
    b_at = case["b_at"]
    s, u = case["scores"][0], case["distinct"][0]
    assert np.array_equal(hb.restated_order(s, u), np.arange(s.size))     # descending, ties by distinct row
    assert case["mult"][u[b_at]] == 2 and case["mult"][u[b_at - 1]] == (2 if mode == "short" else 3)
    held_b, held_r = hb.restated_topk(*hb.expanded(case, 0, upto=b_at), k_out)       # the list when B arrives
    b_rows = case["dup_rows"][case["dup_start"][u[b_at]]:case["dup_start"][u[b_at] + 1]]
    if mode == "short":
      assert held_r[-1] == -1 and held_r[-2] >= 0                          # fewer than k_out entries are held
    else:
      assert held_r[-1] >= 0                                               # exactly k_out are held; the last one ...
      kth = held_b[-1:].view(np.float32)[0]
      assert (kth == s[b_at]) == (mode == "tie") and (mode == "tie" or s[b_at] < kth)
      assert b_rows.max() < held_r[-2]                                     # ... and its neighbour lie above B's rows
    lists[mode] = hb.restated_topk(*hb.expanded(case, 0), k_out)[1]
    changed = not np.array_equal(lists[mode], held_r)
    assert changed == (mode != "lower")                                    # B displaces on the tie, not below it
    if mode == "tie":
      assert set(b_rows.tolist()) <= set(lists[mode].tolist()) and held_r[-1] not in lists[mode]
  assert (b_at // 64 != (b_at - 1) // 64) == (k_out in (66, 130))          # A and B in different groups of 64 results


# ------------------------------------------------------------------------------------------ d. exclude
@pytest.mark.parametrize("kin", hb.EXCLUDE_KIN)
def test_exclude_cases_plant_what_they_say(kin):
  assert 4 * kin * 4 <= 64 * 1024 and (kin < 4096 or 4 * kin * 4 == 64 * 1024)
  ks = hb.exclude_ks(kin)
  assert kin in ks and kin + 3 in ks and (kin == 1 or min(ks) < kin)
  for ne in hb.EXCLUDE_NE:
    case = hb.exclude_case(kin, ne)
    s, ids, ex = case["scores"], case["ids"], case["exclude"]
    assert np.isfinite(s).all() and ex.shape == (5, ne)
    wb, wi, order, isin = hb.exclude_restated(s, ids, ex, kin + 3)
    assert wb.shape == (5, kin)                                            # the width is min(k, kin)
    assert all(np.array_equal(np.sort(order[q]), np.arange(kin)) for q in range(5))
    plain = np.stack([np.lexsort((np.arange(kin), -s[q])) for q in range(5)])
    assert not isin[1].any() and np.array_equal(order[1], plain[1])        # "absent": nothing moves
    if ne == 0:
      assert not isin.any() and np.array_equal(order, plain)
      continue
    assert isin[0].sum() == (kin + 2) // 5 and (kin < 8 or isin[0].sum() >= 2)        # "several": one id, many columns
    assert isin[2].all() and np.array_equal(order[2], plain[2])            # "all": the original order
    # kept columns first, each side in (score descending, column ascending) order
    for q in (0, 3):
      kept = ~isin[q][order[q]]
      n_kept = int(kept.sum())
      assert kept[:n_kept].all() and not kept[n_kept:].any()
    if kin >= 63:
      for side in (True, False):                                           # "ties" on both sides, the lower column first
        cols = order[3][isin[3][order[3]] == side]
        sb = hb.canonical_bits(s[3][cols])
        tied = np.flatnonzero(sb[:-1] == sb[1:])
        assert tied.size and (cols[tied] < cols[tied + 1]).all()
      assert (wb[3] == hb.NEG_ZERO).any() and (wb[3] == 0).any()           # the original bits: -0.0 stays -0.0
      # "outranked": an excluded column stands before a kept one, legitimately
      pos = {int(c): i for i, c in enumerate(order[4])}
      assert isin[4][0] and not isin[4][1] and pos[0] < pos[1] and s[4][1] < s[4][0] - hb.PENALTY
      assert not isin[4][2] and pos[2] < pos[0]
