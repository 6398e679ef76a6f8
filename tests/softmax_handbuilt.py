"""Hand-built batches for the in-batch softmax kernels (csrc/softmax.hip, csrc/softmax16.hip): every builder returns the
two embedding matrices together with what it planted -- the tile that holds each row's maximum, the gap to the next
tile, a ladder of scales -- so a test chooses what the streaming loops see (how many 32-row tiles a wave walks, where
the running maximum moves, how the per-row scale of the backward's T tile has to follow) instead of taking what a
random draw produces.  The two split planners are restated here; tests/test_softmax_handbuilt_host.py proves every
planted property again from the arrays alone, in float64, and the restated geometry against the library's own plan
entry points.  Pure numpy at import; ``entry_point_outputs`` (the one function that touches the GPU) imports torch
when it is called.  Test infrastructure only.

Inputs lie on the grid {-2 .. 2} / 4 unless a builder says otherwise, and every builder keeps to small multiples of
1 / 4: every dot product is then exact in float32 in any summation order, and on the split-fp16 path too (the values
are exact in fp16 under the per-row power-of-two scale, the lo half is 0), so planted maxima and ties are decided on
the device exactly as in float64."""

import numpy as np

TILE = 32
MIN_FLOAT = float(np.float32(np.finfo(np.float32).min / 100.0))


# ------------------------------------------------------------------------------------------ the planners, restated
def _plan(row_blocks, tiles, target):
  """softmax_plan_blocks / the tail of plan16: (nsplit, split_len in rows)."""
  want = max(1, min(tiles, (target + row_blocks - 1) // row_blocks))
  per = (tiles + want - 1) // want
  return (tiles + per - 1) // per, per * TILE


def padded_heads(heads):
  hp = 1
  while hp < heads:
    hp *= 2
  return hp


def plan_f32(nq, heads, nc, waves=None):
  """[nsplit, split_len] of plan_queries (forward, dq: streams the candidates) and of plan_candidates (dc: streams the
  nq * Hp flat head slots) of csrc/softmax.hip under TFRS_SOFTMAX_WAVES = ``waves`` (None: the default 2048)."""
  target = 2048 if waves is None else int(waves)
  qw = TILE // padded_heads(heads)
  qblocks, cblocks = (nq + qw - 1) // qw, (nc + TILE - 1) // TILE
  return list(_plan(qblocks, cblocks, target)) + list(_plan(cblocks, qblocks, target))


def nw_of(n_rows, nw=None):
  return int(nw) if nw is not None and int(nw) in (4, 8) else (8 if n_rows >= 16384 else 4)


def plan_f16(nq, nc, nw=None, wgs=None, wgs_bwd=None):
  """[nsplit, split_len] of the forward, of dq and of dc of csrc/softmax16.hip (plan16) under TFRS_SOFTMAX_NW,
  TFRS_SOFTMAX_WGS and TFRS_SOFTMAX_WGS_BWD (None: auto, 512, 256)."""
  fwd = 512 if wgs is None else int(wgs)
  bwd = 256 if wgs_bwd is None else int(wgs_bwd)

  def one(n_rows, n_stream, target):
    per_wg = nw_of(n_rows, nw) * TILE
    return _plan((n_rows + per_wg - 1) // per_wg, (n_stream + TILE - 1) // TILE, target)
  return list(one(nq, nc, fwd)) + list(one(nq, nc, bwd)) + list(one(nc, nq, bwd))


def split_tiles(n_stream, nsplit, split_len):
  """Tiles each split walks, and the rows of the very last tile, for ``n_stream`` streamed rows."""
  tiles = []
  for sp in range(nsplit):
    lo, hi = sp * split_len, min((sp + 1) * split_len, n_stream)
    assert hi > lo, "an empty split"
    tiles.append((hi - lo + TILE - 1) // TILE)
  return tiles, n_stream - (n_stream - 1) // TILE * TILE


def ring_depth(d):
  """Depth of the backward's LDS ring of csrc/softmax16.hip: 3 for a padded dim <= 64, 2 at 128."""
  return 3 if d <= 64 else 2


# ------------------------------------------------------------------------------------------ builders
def grid(rng, shape):
  return (rng.integers(-2, 3, size=shape) / 4.0).astype(np.float32)


def nonzero_grid(rng, shape):
  """The grid without its 0.  The split-fp16 backward keeps T = w (softmax - onehot) under ONE power-of-two scale per
  owned row, accurate over the upper ~27 binades below that row's largest |T|: a gradient entry is
  accurate relative to its own terms as long as the row's large |T| take part in it.  A batch whose probabilities span
  more than that (every staircase here) must therefore not multiply exactly the large ones by an exact 0 while the tiny
  ones meet a nonzero coordinate -- an entry of 1e-27 made of flushed terms only, beside neighbours of order 1."""
  return (rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape) / 4.0).astype(np.float32)


def option_variants(rng, nq, nc):
  """The logit options of tasks.Retrieval, each alone and all together (as tests/test_multihead_gpu.py draws them)."""
  w = rng.uniform(0.1, 2.0, size=nq).astype(np.float32)
  p = rng.uniform(0.0, 1.0, size=nc).astype(np.float32)
  p[::7] = 0.0                                          # the 1e-6 clip
  ids = rng.integers(0, max(nc // 3, 2), size=nc)       # duplicates: accidental hits
  mask = rng.uniform(size=(nq, nc)) > 0.2
  mask[np.arange(nq), np.arange(nq)] = True
  return {"plain": dict(), "weights": dict(sample_weight=w), "temperature": dict(temperature=0.7),
          "correction": dict(candidate_sampling_probability=p), "accidental_hits": dict(candidate_ids=ids),
          "mask": dict(score_mask=mask),
          "all": dict(sample_weight=w, temperature=1.3, candidate_sampling_probability=p, candidate_ids=ids,
                      score_mask=mask)}


STAIR_Q = 2.0          # coordinate 0 of every query of a staircase
STAIR_NOISE = 4        # coordinates 1 .. 4 carry grid noise (at most 1 in a dot product), the others are 0 in the queries
# step in logit units -> (coordinate 0 of the candidates per level, temperature).  One level is STAIR_Q * c_step in the
# dot product, the noise moves a difference of two dot products by at most 2, the temperatures are powers of two (the
# logits stay exact):
#   8: one level apart [8, 12], five levels at most 60: every probability is a normal float32 and within the fp16 range of
#      the backward's per-row scale;
#   40: one level [56, 72] (below 2^-24 of the new sum, still a normal float32), two levels at least 120;
#   120: one level at least 224.
# No difference falls between 87 and 104, where exp() is a float32 subnormal that a device may flush and float64 keeps:
# from 104 on the probability is exactly 0 on the device and in the oracle's float32 results alike.
STAIR = {8: (5.0, 1.0), 40: (8.0, 0.25), 120: (8.0, 0.0625)}


def tile_levels(kind, ntiles):
  """Level of each candidate tile: ``first`` / ``middle`` / ``last`` plant one tile above the others, ``ascending``
  and ``descending`` are the staircases; an integer plants that tile."""
  if kind == "ascending":
    return np.arange(ntiles)
  if kind == "descending":
    return np.arange(ntiles)[::-1].copy()
  at = {"first": 0, "middle": ntiles // 2, "last": ntiles - 1}.get(kind, kind)
  lv = np.zeros(ntiles, np.int64)
  lv[int(at)] = 1
  return lv


def staircase(nq, nc, d, kind, step=8, seed=0):
  """(q, c, levels, temperature): grid batch whose coordinate 0 carries the planted levels -- queries STAIR_Q, the
  candidates of tile t c_step * level(t) -- so that under ``temperature`` every row's maxima over two tiles one level
  apart differ by at least ``step`` logit units (see STAIR).  The noise is drawn from the grid without 0 (nonzero_grid);
  the queries' coordinates past the noise are 0 in EVERY row, so those gradient entries have no nonzero term at all."""
  c_step, temperature = STAIR[step]
  rng = np.random.default_rng([seed, nq, nc, d])
  q, c = nonzero_grid(rng, (nq, d)), nonzero_grid(rng, (nc, d))
  ntiles = (nc + TILE - 1) // TILE
  levels = tile_levels(kind, ntiles)
  q[:, 1 + STAIR_NOISE:] = 0.0
  q[:, 0] = STAIR_Q
  c[:, 0] = c_step * levels[np.arange(nc) // TILE]
  return q, c, levels, temperature


LADDER_LIKED = (150, 151, 157)     # candidates of the column ladder (no query's positive at the shape it is built for)


def column_ladder(nq, nc, d, ascending=True, seed=0):
  """The staircase seen from the dc side, where a wave owns candidates and streams query tiles: the candidates LADDER_LIKED
  carry 5.25 in coordinate 0 (every other candidate 0.25), the queries of tile t carry -2 (levels below the top) there, so
  their logit for a liked candidate is 10 per level below everyone else's, give or take 2 of grid noise: the probability
  -- |G| of a liked candidate's column -- rises by at least e^8 from one query tile to the next (``ascending``: later
  query tiles like the candidate more; else the reverse)."""
  assert nq <= min(LADDER_LIKED) and max(LADDER_LIKED) < nc
  rng = np.random.default_rng([seed, nq, nc, d, 1])
  q, c = nonzero_grid(rng, (nq, d)), nonzero_grid(rng, (nc, d))
  ntiles = (nq + TILE - 1) // TILE
  below = np.arange(ntiles)[::-1].copy() if ascending else np.arange(ntiles)
  q[:, 1 + STAIR_NOISE:] = 0.0
  c[:, 0] = 0.25                     # (not 0: see nonzero_grid; a common coordinate shifts a whole row of logits)
  c[list(LADDER_LIKED), 0] = 5.25
  q[:, 0] = -2.0 * below[np.arange(nq) // TILE]
  return q, c, below


# ------------------------------------------------------------------------------------------ float64 views of a batch
def logits64(q, c, temperature=None):
  """Plain logits in float64 (exact for the builders above)."""
  s = np.asarray(q, np.float64) @ np.asarray(c, np.float64).T
  return s if temperature is None else s / float(temperature)


def tile_maxima(s):
  """[rows, tiles]: the maximum of every row over each 32-column tile."""
  nt = (s.shape[1] + TILE - 1) // TILE
  return np.stack([s[:, t * TILE:(t + 1) * TILE].max(axis=1) for t in range(nt)], axis=1)


def softmax_g(q, c, temperature=None, sample_weight=None):
  """G = w (softmax - onehot) / T of the plain loss in float64, [nq, nc]."""
  s = logits64(q, c, temperature)
  z = s - s.max(axis=1, keepdims=True)
  p = np.exp(z)
  p /= p.sum(axis=1, keepdims=True)
  g = p - np.eye(*s.shape)
  if sample_weight is not None:
    g = g * np.asarray(sample_weight, np.float64).reshape(-1, 1)
  return g if temperature is None else g / float(temperature)


def row_losses(q, c, sample_weight=None, **kw):
  """(per-row loss lse - pos in float64 without the weight, its yardstick 1 + A_bb + sum_c p_bc A_bc) from the
  oracle's logits; A = |q| |c|^T / |T| is the ``cond`` of oracle/retrieval.py loss_grads."""
  from oracle import retrieval as o_ret
  kw = dict(kw)
  if "candidate_ids" in kw:
    kw["remove_accidental_hits_flag"] = True
  s, _ = o_ret.logits_and_labels(q, c, **kw)
  s = s.astype(np.float64)
  z = s - s.max(axis=1, keepdims=True)
  e = np.exp(z)
  nq = s.shape[0]
  per_row = np.log(e.sum(axis=1)) - z[np.arange(nq), np.arange(nq)]
  p = e / e.sum(axis=1, keepdims=True)
  t = kw.get("temperature")
  a = np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(c, np.float64)).T / (abs(float(t)) if t else 1.0)
  return per_row, 1.0 + a[np.arange(nq), np.arange(nq)] + (p * a).sum(axis=1)


# ------------------------------------------------------------------------------------------ the cases, shared by both tests
# A. streaming depth of the f32 kernels: (TFRS_SOFTMAX_WAVES, heads, (nq, nc, d), forward/dq tiles per split and rows of
#    the last tile, dc tiles per split and rows of the last tile)
F32_DEPTH_CASES = (
    ("1", 1, (33, 70, 20), ([3], 6), ([2], 1)),
    ("1", 1, (97, 97, 64), ([4], 1), ([4], 1)),
    ("1", 1, (5, 225, 8), ([8], 1), ([1], 5)),
    ("2", 1, (20, 150, 16), ([3, 2], 22), ([1], 20)),
    (None, 1, (2048, 2050, 16), ([3] * 21 + [2], 2), ([2] * 32, 32)),
    ("1", 3, (20, 97, 20), ([4], 1), ([3], 16)),
)
# what the suite had before, with the options it ran under: one tile per split everywhere on the f32 kernels
F32_EXISTING_SHAPES = ((2, 2), (64, 64), (100, 333), (257, 300), (512, 512), (1000, 1024))

# C. streaming depth of the split-fp16 kernels under WGS = WGS_BWD = 1: (nq, nc) -> (forward/dq tiles, dc tiles)
F16_DEPTH_SHAPES = {(33, 33): (2, 2), (70, 97): (4, 3), (97, 97): (4, 4), (129, 161): (6, 5), (160, 193): (7, 5),
                    (192, 192): (6, 6), (40, 225): (8, 2)}
F16_DEPTH_DIMS = (20, 64, 100)
# both options at 2: (nq, nc) -> (forward/dq tiles per split, dc tiles per split)
F16_TWO_SPLIT_SHAPES = {(70, 97): ([2, 2], [2, 1]), (97, 225): ([4, 4], [4])}    # 225 owned candidates are two workgroups: one split
# backward tiles per split the suite reached before (the issue's list): no multiple of 3 above 1 ...
F16_EXISTING_BWD_TILES = (1, 2, 5, 16, 128, 2048)

# B. order of the maxima
STAIR_SHAPE = (33, 161, 16)          # 6 candidate tiles
STAIR_KINDS = ("first", "middle", "last", "ascending", "descending")
STAIR_STEPS = (8, 40, 120)

# D. finalize in batches of 16: (nq, nc, d) -> forward splits under the default options
FINALIZE_SHAPES = {(5, 512, 16): 16, (5, 513, 16): 17, (40, 1057, 16): 34}
FINALIZE_GAP = 40


def finalize_plants(nsplit):
  """Splits that hold the row maximum in turn: the first, the first of the second batch of 16 and the last."""
  return sorted({0, min(16, nsplit - 1), nsplit - 1})


# ------------------------------------------------------------------------------------------ the GPU entry points
def entry_point_outputs(q, c, kw, multi_head, reuse=0, with_pos=False):
  """(loss, lse, dq, dc[, pos]) of one forward + backward through the C entry points: the multi-head ones on ``q``
  ([B, H, D], or [B, D] taken as one head: the MH = true kernels) or the 2-D ones on ``q`` [B, D] (the split-fp16
  kernels, or the MH = false kernels under TFRS_SOFTMAX_MODE=f32 and with any logit option).  ``reuse``: the 2-D
  backward takes the operand records the forward left in the workspace."""
  import torch
  from recommenders_amd import _lib
  lib = _lib.load()

  def _t(a, **k):
    return torch.as_tensor(np.asarray(a), **k).cuda()
  q = np.asarray(q, np.float32)
  heads = q.shape[1] if q.ndim == 3 else 1
  nq, d, nc = q.shape[0], q.shape[-1], c.shape[0]
  tq, tc = _t(q), _t(c)
  w = _t(np.asarray(kw["sample_weight"], np.float32)) if "sample_weight" in kw else None
  corr = (torch.log(torch.clamp(_t(kw["candidate_sampling_probability"]), 1e-6, 1.0))
          if "candidate_sampling_probability" in kw else None)
  ids = _t(kw["candidate_ids"]).long() if "candidate_ids" in kw else None
  mask = _t(kw["score_mask"]).to(torch.uint8).contiguous() if "score_mask" in kw else None
  options = (_lib.ptr(w), 1.0 / kw.get("temperature", 1.0), _lib.ptr(corr), _lib.ptr(ids), _lib.ptr(mask))
  shape = (nq, heads, nc, d) if multi_head else (nq, nc, d)
  name = "tfrs_inbatch_softmax_mh_" if multi_head else "tfrs_inbatch_softmax_"
  ws = torch.empty((getattr(lib, name + "workspace_bytes")(*shape),), dtype=torch.uint8, device=tq.device)
  loss, one = torch.empty((), device=tq.device), torch.ones((), device=tq.device)
  lse, pos = torch.empty((nq,), device=tq.device), torch.empty((nq,), device=tq.device)
  dq, dc = torch.empty_like(tq), torch.empty_like(tc)
  stream = _lib.current_stream()
  _lib.check(getattr(lib, name + "ce_fwd")(_lib.ptr(tq), _lib.ptr(tc), *shape, *options, _lib.ptr(loss), _lib.ptr(lse),
                                           _lib.ptr(pos), _lib.ptr(ws), ws.numel(), stream))
  _lib.check(getattr(lib, name + "ce_bwd")(_lib.ptr(tq), _lib.ptr(tc), *shape, *options, _lib.ptr(lse), _lib.ptr(one),
                                           _lib.ptr(dq), _lib.ptr(dc), _lib.ptr(ws), ws.numel(),
                                           *(() if multi_head else (int(reuse),)), stream))
  outs = (loss, lse, dq, dc) + ((pos,) if with_pos else ())
  return tuple(x.detach().cpu().numpy() for x in outs)
