"""Hand-built ScaNN indexes: a ``state_dict`` written array by array (leaf sizes, centres, codebooks, codes, row
permutation, re-ordering rows) that ``ScaNN.load_state_dict`` installs without training and tests/scann_restatement.py
reads, so a test chooses the layout the scan kernels see instead of taking what the k-means trainer produces; and the
assertions that hold a search to the restatement.  Test infrastructure only (no GPU access in the builders)."""

import numpy as np

from oracle import topk as o_topk
from tests import scann_restatement as rs

EDGE_POSITIONS = (0, 31, 32, 127, 128, 4095, 4096, 4097, 8191, 8192)   # in-leaf rows next to a group / range boundary


def min_code_bytes(nb):
  """The layer's code row width for ``nb`` blocks: two codes per byte, rounded up to 4 bytes."""
  return ((nb + 1) // 2 + 3) // 4 * 4


def plant_edges(sizes):
  """[(leaf-major position, kind)]: in every leaf the EDGE_POSITIONS that exist and the last row, kinds 14 / 15
  alternating inside a leaf (the first kind alternates from leaf to leaf), then one more row of the rarer kind (the
  second row of the largest leaf that still has an unplanted one) if the two counts differ: the same number of rows
  per kind."""
  sizes = [int(s) for s in sizes]
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  planted = {}
  for leaf, size in enumerate(sizes):
    j = 0
    for r in EDGE_POSITIONS + (size - 1,):
      if 0 <= r < size and int(off[leaf] + r) not in planted:
        planted[int(off[leaf] + r)] = 15 if (j + leaf) % 2 else 14
        j += 1
  n15 = sum(1 for kind in planted.values() if kind == 15)
  n14 = len(planted) - n15
  assert abs(n15 - n14) <= len(sizes)
  while n14 != n15:
    leaf = max((l for l in range(len(sizes)) if any(int(off[l] + r) not in planted for r in range(sizes[l]))),
               key=lambda l: sizes[l])
    r = next(r for r in range(1, sizes[leaf]) if int(off[leaf] + r) not in planted)
    if n14 < n15:
      planted[int(off[leaf] + r)] = 14
      n14 += 1
    else:
      planted[int(off[leaf] + r)] = 15
      n15 += 1
  return sorted(planted.items())


def build_state(sizes, d, dims_per_block, seed, planted=(), code_bytes=None, rows=False, garbage=False):
  """A ScaNN state dict with leaves of ``sizes`` rows (zeros allowed).

  centroids ~ N(0, 1 / d); perm a random permutation; codebooks [nb, 16, dpb]: codes 0..13 are 0.1 / sqrt(d) * N(0, 1),
  code 15 is 1.0 in the even blocks and 0.0 in the odd ones, code 14 the opposite -- a row whose every block holds 15
  ("kind 15") scores high for a query heavy in the even blocks, low for one heavy in the odd blocks; codes: random
  nibbles in 0..13 except the ``planted`` (leaf-major position, kind) rows, block b in the low (b even) / high (b odd)
  nibble of byte b / 2.  ``code_bytes`` defaults to the layer's minimum and may be larger; with ``garbage`` every byte
  and nibble beyond the nb used ones is random (the search must ignore them; the restatement does).  With ``rows`` the
  state holds rows = f32(mu_leaf + decoded residual), leaf-major, and the corpus c with c[perm] = rows is returned
  beside it: (state, c).  The constructor parameters of the state are num_leaves = len(sizes),
  num_leaves_to_search = len(sizes), no re-ordering and k = 10: ``make_layer`` overrides them."""
  rng = np.random.default_rng(seed)
  sizes = np.asarray(sizes, dtype=np.int64)
  n, num_leaves = int(sizes.sum()), len(sizes)
  dpb = min(int(dims_per_block), int(d))
  nb = (d + dpb - 1) // dpb
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  centroids = (rng.normal(size=(num_leaves, d)) / np.sqrt(d)).astype(np.float32)
  codebooks = (0.1 * rng.normal(size=(nb, 16, dpb)) / np.sqrt(d)).astype(np.float32)
  codebooks[0::2, 15, :], codebooks[1::2, 15, :] = 1.0, 0.0
  codebooks[0::2, 14, :], codebooks[1::2, 14, :] = 0.0, 1.0
  cb = min_code_bytes(nb) if code_bytes is None else int(code_bytes)
  assert cb % 4 == 0 and (nb + 1) // 2 <= cb <= 64, cb
  nib = np.zeros((n, 2 * cb), dtype=np.uint8)
  nib[:, :nb] = rng.integers(0, 14, size=(n, nb))
  for pos, kind in planted:
    nib[pos, :nb] = kind
  if garbage:
    nib[:, nb:] = rng.integers(0, 16, size=(n, 2 * cb - nb))
  codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
  state = dict(centroids=centroids, codebooks=codebooks, codes=codes, leaf_offsets=off,
               perm=rng.permutation(n).astype(np.int32), rows=None, identifiers=None, k=10, num_leaves=num_leaves,
               num_leaves_to_search=num_leaves, training_iterations=0, dimensions_per_block=dpb,
               num_reordering_candidates=None, seed=int(seed))
  if not rows:
    return state
  leaf_of = np.repeat(np.arange(num_leaves), sizes)
  state["rows"] = (centroids[leaf_of].astype(np.float64) + rs.decoded_residuals(state, np.arange(n))).astype(np.float32)
  c = np.empty_like(state["rows"])
  c[state["perm"]] = state["rows"]
  return state, c


def queries(nq, d, dims_per_block, seed):
  """(q [nq, d] f32, even [nq] bool): |N(0, 1)| * 0.05 everywhere plus, on the even blocks (``even``) or the odd ones,
  an amplitude drawn per query and dimension from U(0.5, 1.5).  (With a constant amplitude every query of a kind ranks
  the leaf centres alike and a batch probes two leaf sets.)"""
  rng = np.random.default_rng(seed)
  dpb = min(int(dims_per_block), int(d))
  q = np.abs(rng.normal(size=(nq, d))).astype(np.float32) * np.float32(0.05)
  even = rng.integers(0, 2, size=nq).astype(bool)
  amp = rng.uniform(0.5, 1.5, size=(nq, d)).astype(np.float32)
  block_even = (np.arange(d) // dpb) % 2 == 0
  q += amp * (even[:, None] == block_even[None, :])
  return q, even


def make_layer(state, k, num_leaves_to_search=None, reorder=None):
  """The state installed in a fresh ScaNN layer (needs the GPU).  ``reorder`` = num_reordering_candidates; without it
  the re-ordering rows of the state are left out."""
  from recommenders_amd.layers import factorized_top_k as ftk
  state = dict(state, k=int(k), num_reordering_candidates=reorder)
  if num_leaves_to_search is not None:
    state["num_leaves_to_search"] = int(num_leaves_to_search)
  if reorder is None:
    state["rows"] = None
  else:
    assert state["rows"] is not None, "re-ordering needs build_state(..., rows=True)"
  return ftk.ScaNN(k=int(k), num_leaves=int(state["num_leaves"]), num_leaves_to_search=int(state["num_leaves_to_search"]),
                   num_reordering_candidates=reorder, dimensions_per_block=int(state["dimensions_per_block"])
                   ).load_state_dict(state)


def ordered(scores, rows):
  """True when one query's output is in the result order: score descending, equal scores by ascending row."""
  s, r = np.asarray(scores), np.asarray(rows)
  return bool(np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (r[:-1] < r[1:]))))


def decided_share(state, q, k, num_leaves_to_search):
  """(number of distinct probe sets, mean over the queries of min(k, |surely_in|) / k) of a batch, on the host: how
  much of the answer the restatement's band decides.  A condition on the inputs, not on the kernels."""
  _, _, probe_idx, _ = rs.probes(state, q, k, num_leaves_to_search)
  share = []
  for b in range(len(q)):
    _, s64, eps = rs.candidates(state, q[b], probe_idx[b])
    share.append(min(k, int(rs.surely_in(s64, eps, k).sum())) / k)
  return len({tuple(sorted(p)) for p in probe_idx.tolist()}), float(np.mean(share))


def check_against_restatement(layer, state, q, k, num_leaves_to_search, reorder, scores, rows, corpus=None):
  """The assertions of test_kernels_against_restatement on one call's output (host arrays): the probe plan and the
  probe sets are the restatement's; every returned row lies in a probed leaf and is distinct; without re-ordering each
  s~ is within the header's bound of s64, rows that are surely in the top k are present and every returned row possibly
  is, in the result order; with re-ordering (``reorder`` = R, ``corpus`` the original-order rows) the scores are the
  exact fma chain, in the result order, every returned row is possibly in the approximate top R and the surely-top-R
  rows that beat the k-th result are present.  Returns the mean over the queries of min(k, |surely_in|) / k, the share
  of the answer that the band decides."""
  l_eff, p_max, probe_idx, probe_s = rs.probes(state, q, k, num_leaves_to_search)
  assert layer.probe_plan(k) == (l_eff, p_max)
  got_s, got_leaves = layer.probe_leaves(q, k)
  np.testing.assert_array_equal(got_leaves.cpu().numpy(), probe_idx)
  np.testing.assert_array_equal(got_s.cpu().numpy(), probe_s)
  assert scores.shape == (len(q), k) and rows.shape == (len(q), k)
  exact = o_topk.scores(q, corpus) if reorder is not None else None
  share = []
  for b in range(len(q)):
    orig, s64, eps = rs.candidates(state, q[b], probe_idx[b])
    share.append(min(k, int(rs.surely_in(s64, eps, k).sum())) / k)
    where = {int(r): j for j, r in enumerate(orig)}
    assert len(set(rows[b].tolist())) == k, b
    assert all(int(r) in where for r in rows[b]), (b, "a returned row is outside the probed leaves")
    j = np.asarray([where[int(r)] for r in rows[b]])
    assert ordered(scores[b], rows[b]), b
    if reorder is None:
      err = np.abs(scores[b].astype(np.float64) - s64[j])
      assert np.all(err <= eps[j]), (b, rows[b][err > eps[j]].tolist(), float((err / eps[j]).max()))
      sure = np.flatnonzero(rs.surely_in(s64, eps, k))
      assert set(orig[sure].tolist()) <= set(rows[b].tolist()), b
      assert np.all(rs.possibly_in(s64, eps, k)[j]), b
    else:
      r_eff = min(max(k, reorder), len(orig))
      np.testing.assert_array_equal(scores[b], exact[b, rows[b]])
      assert np.all(rs.possibly_in(s64, eps, r_eff)[j]), b
      sure = rs.surely_in(s64, eps, r_eff)
      kth = (-float(scores[b, -1]), int(rows[b, -1]))
      better = [int(orig[t]) for t in np.flatnonzero(sure) if (-float(exact[b, orig[t]]), int(orig[t])) < kth]
      assert set(better) <= set(rows[b].tolist()), b
  return float(np.mean(share))
