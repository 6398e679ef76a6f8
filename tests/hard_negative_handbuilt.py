"""Hand-built batches for the mined in-batch softmax kernels (test infrastructure only).

Embeddings are integer valued (entries in -3 .. 3, or the special rows of ``division_case``), so every dot product is
exact in float32 in any summation order; temperatures are None, 0.5, 2 and 1.5, corrections are multiples of 1/8 given
as the log values of the C ABI.  ``hard_negative_restatement.logits(exact_f32=True)`` then reproduces the device's
logits bit for bit, and with them the kept set, ``(tau, cut)`` and the rank counts.

``planted`` lists, per case, the rows whose cut column was placed by hand: ``(row, cut)``.  Such a row's query has no
zero entry and a group of candidates equal to ``3 * sign(q_row)``, the largest dot product any candidate in the range
can reach with it; with more copies than ``n`` the row takes the lowest ``n`` of them."""

import numpy as np

from tests import hard_negative_restatement as hn

TEMPERATURES = (None, 0.5, 2.0, 1.5)
GPU_TEST_WAVES = "4096"      # TFRS_SOFTMAX_WAVES of the GPU tests: every candidate tile of these shapes is a split


def _ints(rng, shape):
  return rng.integers(-3, 4, size=shape).astype(np.float32)


def _corr(rng, nc):
  return (rng.integers(-16, 17, size=nc) / 8.0).astype(np.float32)


def _plant(q, c, row, cols, signs):
  q[row] = signs
  c[list(cols)] = 3.0 * np.sign(signs)


def small_case(n, temperature=None, with_corr=False):
  """(5, 7, 3): dots in -27 .. 27 over 35 pairs -- ties in nearly every row; n = 0, 1, 3, 5, 6 = nc - 1 and 50."""
  rng = np.random.default_rng(70)
  q, c = _ints(rng, (5, 3)), _ints(rng, (7, 3))
  return dict(name=f"small-n{n}-T{temperature}-corr{int(with_corr)}", q=q, c=c, n=n, temperature=temperature,
              log_corr=_corr(rng, 7) if with_corr else None, ids=None, mask=None, planted=[])


def tile_edge_case(temperature=None):
  """(33, 70, 8), n = 4: the cut falls between tile rows 3 and 4 (the two lane halves: row 10, cut 3), between rows
  31 and 32 (two tiles, and two splits when every tile is a split: row 20, cut 31) and in the third split after two
  ties of the second (row 5: copies at 50, 60 | 64 .. 67, cut 65)."""
  rng = np.random.default_rng(71)
  q, c = _ints(rng, (33, 8)), _ints(rng, (70, 8))
  _plant(q, c, 10, range(0, 6), np.array([3, 3, 3, 3, 3, 3, 3, 3], np.float32))
  _plant(q, c, 20, range(28, 34), np.array([3, -3, 3, -3, 3, -3, 3, -3], np.float32))
  _plant(q, c, 5, (50, 60, 64, 65, 66, 67), np.array([-3, -3, 3, 3, -3, -3, 3, 3], np.float32))
  return dict(name=f"tile-edges-T{temperature}", q=q, c=c, n=4, temperature=temperature, log_corr=None, ids=None,
              mask=None, planted=[(10, 3), (20, 31), (5, 65)])


def duplicated_case(temperature=None, accidental_hits=False):
  """(64, 200, 16), n = 17: candidates 100 .. 139 are copies of 0 .. 39, so every row holds 40 tied pairs, five
  tiles apart.  With ``accidental_hits`` a copy carries its original's id: for rows 0 .. 39 the copy of the positive
  is an accidental hit (MIN_FLOAT)."""
  rng = np.random.default_rng(72)
  q, c = _ints(rng, (64, 16)), _ints(rng, (200, 16))
  c[100:140] = c[0:40]
  ids = None
  if accidental_hits:
    ids = np.arange(200, dtype=np.int64)
    ids[100:140] = ids[0:40]
  return dict(name=f"duplicated-T{temperature}-hits{int(accidental_hits)}", q=q, c=c, n=17, temperature=temperature,
              log_corr=None, ids=ids, mask=None, planted=[])


def mask_case(d, temperature=None):
  """(40, 96, d), d = 5 or 100 (no 16-byte row loads), n = 6, correction and mask: row 7's mask is all False (every
  logit MIN_FLOAT, the lowest six negatives are taken, loss log 7), row 9 has two unmasked negatives (30 and 70), the
  rest is masked at random with the positive kept."""
  rng = np.random.default_rng(73 + d)
  q, c = _ints(rng, (40, d)), _ints(rng, (96, d))
  mask = rng.uniform(size=(40, 96)) > 0.3
  mask[np.arange(40), np.arange(40)] = True
  mask[7] = False
  mask[9] = False
  mask[9, [9, 30, 70]] = True
  return dict(name=f"mask-d{d}-T{temperature}", q=q, c=c, n=6, temperature=temperature, log_corr=_corr(rng, 96),
              ids=None, mask=mask, planted=[(7, 5), (9, 3)])


def division_case():
  """q = (4096, 1), positive (3072, 1): dot 12582913; a negative (3072, 2): dot 12582914; T = 1.5.  Both quotients
  round to 8388609.0, so the negative does not outrank the positive; a multiplication by the rounded reciprocal gives
  8388609 and 8388610."""
  q = np.array([[4096, 1], [1, 0]], np.float32)
  c = np.array([[3072, 1], [0, 1], [3072, 2]], np.float32)
  return dict(name="division", q=q, c=c, n=None, temperature=1.5, log_corr=None, ids=None, mask=None, planted=[])


def selection_cases():
  cases = [small_case(n, t, corr) for n in (0, 1, 3, 5, 6, 50) for t, corr in ((None, False), (1.5, True))]
  cases += [small_case(3, 0.5), small_case(3, 2.0, True)]
  cases += [tile_edge_case(t) for t in (None, 1.5)]
  cases += [duplicated_case(None, False), duplicated_case(0.5, True), duplicated_case(1.5, True)]
  cases += [mask_case(5, None), mask_case(5, 2.0), mask_case(100, 1.5)]
  return cases


def expected(case):
  """Exact float32 logits of the case and what follows from them: kept set, (tau, cut), counts."""
  s = hn.logits(case["q"], case["c"], temperature=case["temperature"], log_corr=case["log_corr"],
                candidate_ids=case["ids"], score_mask=case["mask"], exact_f32=True)
  out = dict(s=s)
  if case["n"] is None:
    out["keep"] = hn.kept_set(s, None)
  else:
    out["keep"] = hn.kept_set(s, case["n"])
    out["tau"], out["cut"] = hn.tau_cut(s, case["n"])
  out["counts"], out["finite"] = hn.rank_counts(s, out["keep"])
  return out
