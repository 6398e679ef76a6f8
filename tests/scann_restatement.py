"""Float64 NumPy restatement of the ScaNN search (recommenders_amd/layers/factorized_top_k/scann.py ``ScaNN``), working from
a layer's ``state_dict``: probe sets with ``L_eff``, the approximate score s~ of the decoded vectors with the error
bound of include/tfrs_hip.h, and the band-aware checks of a returned top-k.  Test infrastructure only."""

import numpy as np

from oracle import topk as o_topk


def decoded_residuals(state, positions):
  """r^ [len(positions), d] (float64) of leaf-major positions: codebook value of each block's 4-bit code."""
  cb = np.asarray(state["codebooks"], dtype=np.float64)          # [nb, 16, dpb]
  nb, _, dpb = cb.shape
  d = state["centroids"].shape[1]
  codes = np.asarray(state["codes"])[positions]                    # [m, code_bytes]
  blocks = np.arange(nb)
  nib = (codes[:, blocks // 2] >> (4 * (blocks % 2))) & 15         # [m, nb]
  r = cb[blocks[None, :], nib]                                     # [m, nb, dpb]
  return r.reshape(len(positions), nb * dpb)[:, :d]


def probe_width(sizes, num_leaves_to_search, k):
  """(L_eff, P_max) by the definition, one candidate width at a time: the smallest L' >= num_leaves_to_search
  (clipped to the leaf count) whose L' smallest leaves hold k rows, and the rows of the L_eff largest leaves."""
  sizes = sorted(int(s) for s in sizes)
  l_eff = max(1, min(int(num_leaves_to_search), len(sizes)))
  while sum(sizes[:l_eff]) < k:
    l_eff += 1
    assert l_eff <= len(sizes), "fewer than k rows in the index"
  return l_eff, sum(sizes[::-1][:l_eff])


def probes(state, queries, k, num_leaves_to_search):
  """(L_eff, P_max, probe lists [B, L_eff] in score order, leaf scores) of the leaf pass: exact top-L_eff of q . mu
  under (score desc, leaf asc) with the d-ordered f32 fma chain."""
  sizes = np.diff(np.asarray(state["leaf_offsets"]))
  l_eff, p_max = probe_width(sizes, num_leaves_to_search, k)
  s, idx = o_topk.brute_force(np.asarray(queries, np.float32), np.asarray(state["centroids"], np.float32), l_eff)
  return l_eff, p_max, idx, s


def candidates(state, query, probe_list):
  """(original rows, s64, eps) of every row of the probed leaves of ONE query: s64 = q . (mu_leaf + r^) in float64,
  eps the bound of include/tfrs_hip.h on |s~ - s64|."""
  off = np.asarray(state["leaf_offsets"])
  perm = np.asarray(state["perm"])
  mu = np.asarray(state["centroids"], dtype=np.float64)
  q = np.asarray(query, dtype=np.float64)
  cmax = float(np.abs(np.asarray(state["codebooks"], dtype=np.float64)).max())
  d = q.shape[0]
  pos, leaf_of = [], []
  for leaf in probe_list:
    p = np.arange(off[leaf], off[leaf + 1])
    pos.append(p)
    leaf_of.append(np.full(len(p), leaf))
  pos = np.concatenate(pos)
  leaf_of = np.concatenate(leaf_of)
  r = decoded_residuals(state, pos)
  m = mu[leaf_of]
  s64 = (m + r) @ q
  eps = 2.0 ** -9 * ((np.abs(m) + np.abs(r)) @ np.abs(q)) + 2.0 ** -32 * d * np.abs(q).max() * cmax
  return perm[pos], s64, eps


def surely_in(s64, eps, m):
  """Rows that are in the top m of s~ whatever s~ is within the band: fewer than m OTHER rows can reach them."""
  hi = np.sort(s64 + eps)
  lo = s64 - eps
  reach = len(hi) - np.searchsorted(hi, lo, side="left") - 1      # others with hi >= lo (minus the row itself)
  return reach < m


def possibly_in(s64, eps, m):
  """Rows that can be in the top m of s~ for some s~ within the band: fewer than m rows surely beat them."""
  lo = np.sort(s64 - eps)
  hi = s64 + eps
  beat = len(lo) - np.searchsorted(lo, hi, side="right")           # rows with lo > hi
  return beat < m
