// softmax_shared.h -- what the in-batch softmax translation units share (softmax.hip: the f32-MFMA loss kernels;
// softmax_mined.hip: the same loss over a mined / adjusted kept set): the kernel argument block, the logit
// function, the two tile loops every f32 kernel of either file is an instance of (softmax_stream_queries: a wave
// owns queries and hands each tile of logits to a consumer; softmax_bwd_body: the gradient kernels), the online
// softmax consumer, the split planner (TFRS_SOFTMAX_WAVES), the workspace carving, the finalize and
// partial-gradient reduce kernels and their launchers.  The tile loops are device function templates over a POLICY
// -- the logit function, the keep predicate and the per-query row state (tau, cut) it reads -- so the prefetch, the
// LDS mirror and the second GEMM exist once in the source; each kernel is its own instantiation (the compiler
// allocates registers per instance: the instances of two policies are not instruction-identical).  Host helpers
// and the small kernels are `static`: each translation unit carries its own copy, nothing is exported.
#pragma once

#include <algorithm>
#include <type_traits>

#include <stdlib.h>

#include "mfma_tile.h"

namespace tfrs {

constexpr float kMinFloat = -3.4028234663852886e36f;  // np.finfo(float32).min / 100

struct SoftmaxArgs {
  const float *q, *c;
  int64_t nq, nc;
  int d;
  const float *w;       // [nq] sample weights or NULL
  float inv_t;          // 1 / temperature
  const float *corr;    // [nc] log(clip(p, 1e-6, 1)) or NULL
  const int64_t *ids;   // [nc] candidate ids (accidental-hit removal) or NULL
  const uint8_t *mask;  // [nq, nc] score_mask or NULL
  int nsplit;
  int64_t split_len;    // multiple of 32
  float *pm, *pl;       // [nsplit, nq] partial max / sum-exp
  float *ppos;          // [nq] positive logit
  const float *lse;     // [nq]
  const float *gloss;   // device scalar or NULL (= 1)
  float *partial;       // [nsplit, rows, d] partial gradients
  uint32_t *ticket;     // finalize kernel's arrival counter (re-armed by the forward kernel)
  int heads;            // H (the MH = false kernels do not read it: 1)
  int lhp;              // log2(Hp)  (... 0)
};

__device__ __forceinline__ float make_logit(float dot, int64_t query, int64_t cand,
                                            const SoftmaxArgs &a, float corr_c,
                                            int64_t id_q, int64_t id_c, bool *masked) {
  float v = dot * a.inv_t;
  if (a.corr) v -= corr_c;
  if (a.ids && cand != query && id_c == id_q) v += kMinFloat;
  *masked = false;
  if (a.mask && !a.mask[query * a.nc + cand]) {
    v = kMinFloat;
    *masked = true;
  }
  return v;
}

// The policy of the plain loss: make_logit, every column kept, no per-query state.  A policy supplies
//   logit(dot, query, cand, corr_c, id_q, id_c, &masked)   make_logit's signature without the args
//   keep(v, query, cand, row)                              does the logit v of (query, cand) enter the softmax
//   row(query)                                             what keep() reads per query (Row{}: an invalid row)
struct PlainPolicy {
  const SoftmaxArgs &a;
  struct Row {};
  __device__ __forceinline__ float logit(float dot, int64_t query, int64_t cand, float corr_c, int64_t id_q,
                                         int64_t id_c, bool *masked) const {
    return make_logit(dot, query, cand, a, corr_c, id_q, id_c, masked);
  }
  __device__ __forceinline__ Row row(int64_t) const { return {}; }
  __device__ static __forceinline__ bool keep(float, int64_t, int64_t, Row) { return true; }
};

// Head max where a query's heads are the Hp adjacent lanes of a group (forward, dq): every lane of the group
// ends with the same value (all lanes take part).  WINNER: *lowest = this lane (head slot hs) is the lowest
// head slot of its group that attains the max.
template <bool WINNER>
__device__ __forceinline__ float head_max_lanes(float own, int hp, int lane, int hs, bool *lowest) {
  float v = own;
  for (int x = 1; x < hp; x <<= 1) v = fmaxf(v, __shfl_xor(v, x));
  if constexpr (WINNER) {
    const uint32_t field = hp == 32 ? 0xFFFFFFFFu : ((1u << hp) - 1u);
    const uint64_t tied = __ballot(own == v);
    const uint32_t grp = (uint32_t)(tied >> (lane - hs)) & field;  // bit s: head slot s attains the max
    *lowest = (grp & (0u - grp)) == (1u << hs);
  }
  return v;
}

// (v2, i2) beats (v1, i1): larger value, or the same value at a lower head index
__device__ __forceinline__ void take_better(float &v1, int &i1, float v2, int i2) {
  const bool t = v2 > v1 || (v2 == v1 && i2 < i1);
  v1 = t ? v2 : v1;
  i1 = t ? i2 : i1;
}

// Head max where a query's heads are the Hp adjacent tile rows (dc): on return every register of a query's
// group holds the group's max in best[] and its lowest head slot in bi[].  Tile row bits 0, 1 are register
// bits 0, 1; bit 2 is the lane half; bits 3, 4 are register bits 2, 3.
__device__ __forceinline__ void head_max_regs(float (&best)[16], int (&bi)[16], int lhp) {
#pragma unroll
  for (int stage = 0; stage < 5; ++stage) {
    if (lhp <= stage) continue;
    if (stage == 2) {  // tile rows t and t ^ 4 are the two lane halves
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ov = __shfl_xor(best[r], 32);
        const int oi = __shfl_xor(bi[r], 32);
        take_better(best[r], bi[r], ov, oi);
      }
    } else {
      const int bit = stage < 2 ? 1 << stage : 1 << (stage - 1);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!(r & bit)) {
          take_better(best[r], bi[r], best[r | bit], bi[r | bit]);
          best[r | bit] = best[r];
          bi[r | bit] = bi[r];
        }
    }
  }
}

// What a lane of a wave that owns queries (softmax_stream_queries) knows: the args, its query and its split.
template <class Row>
struct QueryLane {
  const SoftmaxArgs &a;
  int lane, j, h;   // lane, lane & 31 (the owned flat row), lane >> 5 (the lane half: which 16 rows of a tile)
  int hs, sp;       // head slot of the owned row (MH = false: 0), split of the candidates
  int64_t qb, query, id_q;
  bool qvalid;
  Row row;          // the policy's per-query state, hoisted
};

// The forward tile loop: the wave (WAVES per workgroup) owns 32 / Hp queries as the MFMA B operand and streams the
// 32-candidate tiles of its split one tile ahead; every logit of a tile goes to the consumer:
//   begin(w, bq) -> bool             once, with the owned fragment; false: the wave leaves (wave-uniform)
//   element(w, r, cand, valid, v)    accumulator register r = the logit v of (w.query, cand); !valid: v = -inf
//   tile_end(w, c0), finish(w)       after the 16 elements of the tile at candidate c0; after the last tile
template <int DP, bool MH, int WAVES, class Policy, class Consumer>
__device__ __forceinline__ void softmax_stream_queries(const SoftmaxArgs &a, const Policy &pol, Consumer &con) {
  QueryLane<typename Policy::Row> w{a};
  w.lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lhp = MH ? a.lhp : 0, heads = MH ? a.heads : 1;
  const int hp = 1 << lhp, qw = 32 >> lhp;  // head slots per query, queries per wave
  const int64_t wid = (int64_t)blockIdx.x * WAVES + wave;
  const int64_t nqb = (a.nq + qw - 1) / qw;
  if (wid >= nqb * a.nsplit) return;
  w.qb = wid / a.nsplit;
  w.sp = (int)(wid - w.qb * a.nsplit);
  const int j = w.j = w.lane & 31, h = w.h = w.lane >> 5;
  w.hs = j & (hp - 1);
  w.query = w.qb * qw + (j >> lhp);
  w.qvalid = w.query < a.nq;
  const bool rvalid = w.qvalid && w.hs < heads;
  const bool vec_ok = (a.d == DP) && ((((uintptr_t)a.q) | ((uintptr_t)a.c)) % 16 == 0);
  if (w.qvalid) w.row = pol.row(w.query);

  float bq[DP / 2];
  load_row_frag<DP>(bq, a.q, w.query * heads + w.hs, rvalid, a.d, h, vec_ok);
  w.id_q = (a.ids && w.qvalid) ? a.ids[w.query] : 0;
  if (!con.begin(w, bq)) return;

  const int64_t c_lo = (int64_t)w.sp * a.split_len;
  int64_t c_hi = c_lo + a.split_len;
  if (c_hi > a.nc) c_hi = a.nc;

  // the next tile's fragment is fetched while the current one is multiplied
  float af_next[DP / 2];
  load_row_frag<DP>(af_next, a.c, c_lo + j, c_lo + j < a.nc && c_lo < c_hi, a.d, h, vec_ok);
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) af[s] = af_next[s];
    if (c0 + 32 < c_hi) load_row_frag<DP>(af_next, a.c, c0 + 32 + j, c0 + 32 + j < a.nc, a.d, h, vec_ok);
    const f32x16 acc = tile_dot<DP>(af, bq);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float dot = acc[r];
      if constexpr (MH) dot = head_max_lanes<false>(rvalid ? acc[r] : -__builtin_inff(), hp, w.lane, w.hs, nullptr);
      const int64_t cand = c0 + tile_row_of_reg(r, h);
      const bool valid = w.qvalid && cand < c_hi;
      float v = -__builtin_inff();
      bool masked;
      if (valid)
        v = pol.logit(dot, w.query, cand, a.corr ? a.corr[cand] : 0.0f, w.id_q, a.ids ? a.ids[cand] : 0, &masked);
      con.element(w, r, cand, valid, v);
    }
    con.tile_end(w, c0);
  }
  con.finish(w);
}

// The consumer of the loss forward: the online (max, sum-exp) of the kept logits of a query over its split and the
// positive logit; writes pm / pl per (split, query) and ppos.  Every lane of a head group carries the same (m, l).
template <class Policy>
struct OnlineSoftmax {
  using Lane = QueryLane<typename Policy::Row>;
  float m = -__builtin_inff(), l = 0.0f, pos = 0.0f, tmax = -__builtin_inff();
  bool haspos = false;
  float s[16];

  template <class Frag>
  __device__ __forceinline__ bool begin(const Lane &w, const Frag &) {
    // re-arms the finalize kernel's ticket: it runs strictly after this kernel (a hipMemsetAsync
    // node is not reliably ordered against kernel nodes when the step replays from a HIP graph)
    if (blockIdx.x == 0 && threadIdx.x == 0) *w.a.ticket = 0u;
    return true;
  }
  __device__ __forceinline__ void element(const Lane &w, int r, int64_t cand, bool valid, float v) {
    float kept = -__builtin_inff();
    if (valid) {
      if (Policy::keep(v, w.query, cand, w.row)) kept = v;
      if (cand == w.query) {
        pos = v;
        haspos = true;
      }
    }
    s[r] = kept;
    tmax = fmaxf(tmax, kept);
  }
  __device__ __forceinline__ void tile_end(const Lane &, int64_t) {
    if (tmax > m) {
      l *= __expf(m - tmax);  // m = -inf on the first tile: exp(-inf) = 0, l = 0
      m = tmax;
    }
    if (m > -__builtin_inff()) {
#pragma unroll
      for (int r = 0; r < 16; ++r) l += __expf(s[r] - m);  // s = -inf contributes 0
    }
    tmax = -__builtin_inff();
  }
  __device__ __forceinline__ void finish(const Lane &w) {
    // the two lane halves hold disjoint candidates of the same query
    const float m2 = __shfl_xor(m, 32), l2 = __shfl_xor(l, 32);
    const float mm = fmaxf(m, m2);
    float ll = 0.0f;
    if (m > -__builtin_inff()) ll += l * __expf(m - mm);
    if (m2 > -__builtin_inff()) ll += l2 * __expf(m2 - mm);
    if (w.h == 0 && w.hs == 0 && w.qvalid) {
      w.a.pm[(int64_t)w.sp * w.a.nq + w.query] = mm;
      w.a.pl[(int64_t)w.sp * w.a.nq + w.query] = ll;
    }
    if (haspos && w.hs == 0) w.a.ppos[w.query] = pos;  // one lane of one split: head slot 0 of the half that sees c = b
  }
};

// The gradient tile loop, four waves per workgroup; `smem`: 4 * 32 * (DP + 4) floats of dynamic LDS.
// ROWS_ARE_QUERIES = true : wave owns 32 / Hp queries (32 flat rows), streams candidates, partial dq.
// ROWS_ARE_QUERIES = false: wave owns 32 candidates, streams the flat rows (slot space: query * Hp + head
//                           slot, a tile = 32 / Hp whole queries), partial dc.
template <int DP, bool ROWS_ARE_QUERIES, bool MH, class Policy>
__device__ __forceinline__ void softmax_bwd_body(const SoftmaxArgs &a, const Policy &pol, float *smem) {
  using Row = typename Policy::Row;
  constexpr int NFB = (DP + 31) / 32;  // 32-feature output blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lhp = MH ? a.lhp : 0, heads = MH ? a.heads : 1;
  const int hp = 1 << lhp, qw = 32 >> lhp;
  const int64_t nslots = a.nq << lhp;
  const int64_t nrb = ROWS_ARE_QUERIES ? (a.nq + qw - 1) / qw : (a.nc + 31) / 32;
  const int64_t n_s = ROWS_ARE_QUERIES ? a.nc : nslots;
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  if (wid >= nrb * a.nsplit) return;
  const int64_t rb = wid / a.nsplit;
  const int sp = (int)(wid - rb * a.nsplit);
  const int j = lane & 31, h = lane >> 5;
  const bool vec_ok = (a.d == DP) && ((((uintptr_t)a.q) | ((uintptr_t)a.c)) % 16 == 0);

  // the owned row: a flat (query, head) row or a candidate
  const int hs_own = j & (hp - 1);
  const int64_t q_own = rb * qw + (j >> lhp);
  const int64_t rrow = ROWS_ARE_QUERIES ? q_own * heads + hs_own : rb * 32 + j;  // row of q / of c, and of the output
  const bool rvalid = ROWS_ARE_QUERIES ? (q_own < a.nq && hs_own < heads) : (rrow < a.nc);

  float br[DP / 2];
  load_row_frag<DP>(br, ROWS_ARE_QUERIES ? a.q : a.c, rrow, rvalid, a.d, h, vec_ok);

  // per-lane constants of the owned row
  float lse_r = 0.0f, w_r = 1.0f, corr_r = 0.0f;
  int64_t id_r = 0;
  Row row_r;
  if (rvalid) {
    if (ROWS_ARE_QUERIES) {
      lse_r = a.lse[q_own];
      if (a.w) w_r = a.w[q_own];
      if (a.ids) id_r = a.ids[q_own];  // nq <= nc, so a query is also a valid candidate row
      row_r = pol.row(q_own);
    } else {
      if (a.corr) corr_r = a.corr[rrow];
      if (a.ids) id_r = a.ids[rrow];
    }
  }
  const float gl = (a.gloss ? *a.gloss : 1.0f) * a.inv_t;

  f32x16 outacc[NFB];
#pragma unroll
  for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
    for (int r = 0; r < 16; ++r) outacc[fb][r] = 0.0f;

  const int64_t s_lo = (int64_t)sp * a.split_len;
  int64_t s_hi = s_lo + a.split_len;
  if (s_hi > n_s) s_hi = n_s;

  // Streamed tile (32 rows x DP features): fetched one tile ahead into registers (row j, half h
  // = the first GEMM's A fragment) and mirrored into this wave's LDS slab so that the second
  // GEMM can read it transposed (lane = feature) with conflict-free ds_read_b32.
  constexpr int kLd = DP + 4;  // floats per LDS row (+16 B: rows start in different bank groups)
  float *slab = smem + (size_t)wave * 32 * kLd;
  float af_next[DP / 2];
  // lane j's row of the tile at s0 = u - j: candidate u, or the flat row of slot u (head slots >= H hold zeros)
  auto fetch = [&](int64_t u, bool more) {
    const int hs = ROWS_ARE_QUERIES ? 0 : (int)(u & (hp - 1));
    const int64_t row = ROWS_ARE_QUERIES ? u : (u >> lhp) * heads + hs;
    load_row_frag<DP>(af_next, ROWS_ARE_QUERIES ? a.c : a.q, row, more && u < n_s && hs < heads, a.d, h, vec_ok);
  };
  fetch(s_lo + j, s_lo < s_hi);

  for (int64_t s0 = s_lo; s0 < s_hi; s0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) af[s] = af_next[s];
    if (s0 + 32 < s_hi) fetch(s0 + 32 + j, true);
#pragma unroll
    for (int m4 = 0; m4 < DP / 8; ++m4)
      *reinterpret_cast<float4 *>(slab + j * kLd + h * (DP / 2) + 4 * m4) =
          make_float4(af[4 * m4], af[4 * m4 + 1], af[4 * m4 + 2], af[4 * m4 + 3]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x16 acc = tile_dot<DP>(af, br);

    // head max and its lowest head per (query, candidate) pair; `win[r]`: this element is that head
    float best[16];
    bool win[16];
    if constexpr (!MH) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        best[r] = acc[r];
        win[r] = rvalid && s0 + tile_row_of_reg(r, h) < s_hi;
      }
    } else if constexpr (ROWS_ARE_QUERIES) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        bool lowest;
        best[r] = head_max_lanes<true>(rvalid ? acc[r] : -__builtin_inff(), hp, lane, hs_own, &lowest);
        win[r] = rvalid && s0 + tile_row_of_reg(r, h) < s_hi && lowest;
      }
    } else {
      int bi[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tile_row_of_reg(r, h);
        const int hs = t & (hp - 1);
        const bool valid = rvalid && s0 + t < s_hi && hs < heads;
        best[r] = valid ? acc[r] : -__builtin_inff();
        bi[r] = hs;
      }
      head_max_regs(best, bi, lhp);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tile_row_of_reg(r, h);
        const int hs = t & (hp - 1);
        win[r] = rvalid && s0 + t < s_hi && hs < heads && bi[r] == hs;
      }
    }

    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float gg = 0.0f;
      if (win[r]) {
        const int64_t srow = s0 + tile_row_of_reg(r, h);
        const int64_t query = ROWS_ARE_QUERIES ? q_own : (srow >> lhp);
        const int64_t cand = ROWS_ARE_QUERIES ? srow : rrow;
        const float corr_c = ROWS_ARE_QUERIES ? (a.corr ? a.corr[cand] : 0.0f) : corr_r;
        const int64_t id_q = ROWS_ARE_QUERIES ? id_r : (a.ids ? a.ids[query] : 0);
        const int64_t id_c = ROWS_ARE_QUERIES ? (a.ids ? a.ids[cand] : 0) : id_r;
        bool masked;
        const float v = pol.logit(best[r], query, cand, corr_c, id_q, id_c, &masked);
        const Row row_q = ROWS_ARE_QUERIES ? row_r : pol.row(query);
        if (!masked && Policy::keep(v, query, cand, row_q)) {
          const float lse_q = ROWS_ARE_QUERIES ? lse_r : a.lse[query];
          const float w_q = ROWS_ARE_QUERIES ? w_r : (a.w ? a.w[query] : 1.0f);
          gg = w_q * (__expf(v - lse_q) - (cand == query ? 1.0f : 0.0f)) * gl;
        }
      }
      g[r] = gg;
    }

    // out^T[feature][owned row] += sum over the 32 streamed rows of X[srow][feature] * G[srow][row]
    // MFMA step r contracts the streamed-row pair (tile_row_of_reg(r,0), tile_row_of_reg(r,1)),
    // which is exactly where g[r] lives in lane halves 0 / 1.  Rows past the end and padded
    // features are zero in the slab.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *xrow = slab + tile_row_of_reg(r, h) * kLd;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        const int feat = fb * 32 + j;
        const float av = (feat < DP) ? xrow[feat] : 0.0f;
        outacc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, g[r], outacc[fb], 0, 0, 0);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the slab is rewritten by the next tile
  }

  if (rvalid) {
    const int64_t n_out = ROWS_ARE_QUERIES ? a.nq * heads : a.nc;
    float *dst = a.partial + ((int64_t)sp * n_out + rrow) * a.d;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int feat = fb * 32 + tile_row_of_reg(r, h);
        if (feat < a.d) dst[feat] = outacc[fb][r];
      }
  }
}

// Combines the per-split (max, sum) pairs, writes lse/pos and the weighted loss.
// One thread per query row; every block leaves a partial loss in block_part[] and the LAST
// block to finish (ticket counter) adds the partials in block order, so the result does not
// depend on scheduling.  `ticket` must be zero on entry and is reset for the next launch.
static __global__ void __launch_bounds__(256) softmax_finalize_kernel(const SoftmaxArgs a, float *out_loss,
                                                               float *out_lse, float *out_pos,
                                                               double *block_part, uint32_t *ticket) {
  __shared__ double red[256];
  __shared__ bool is_last;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double local = 0.0;
  if (row < a.nq) {
    float mm = -__builtin_inff();
    for (int sp = 0; sp < a.nsplit; ++sp) mm = fmaxf(mm, a.pm[(int64_t)sp * a.nq + row]);
    float ll = 0.0f;
    for (int sp = 0; sp < a.nsplit; ++sp) {
      const float pm = a.pm[(int64_t)sp * a.nq + row];
      if (pm > -__builtin_inff()) ll += a.pl[(int64_t)sp * a.nq + row] * expf(pm - mm);
    }
    const float lse = mm + logf(ll);
    const float pos = a.ppos[row];
    out_lse[row] = lse;
    out_pos[row] = pos;
    const float w = a.w ? a.w[row] : 1.0f;
    // (mm - pos) + log(ll), not lse - pos: for a row whose score_mask is all False mm and pos are both kMinFloat, whose
    // ulp (2.5e29) swallows log(ll) in lse -- the difference first is exact there and the row's loss is log(nc)
    local = (double)w * ((double)(mm - pos) + (double)logf(ll));
  }
  red[threadIdx.x] = local;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&block_part[blockIdx.x], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = (t == gridDim.x - 1);
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double total = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b)
      total += __hip_atomic_load(&block_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *out_loss = (float)total;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static __global__ void __launch_bounds__(256) reduce_partials_kernel(const float *partial, int nsplit,
                                                              int64_t count, float *out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count;
       t += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.0f;
    for (int sp = 0; sp < nsplit; ++sp) acc += partial[(int64_t)sp * count + t];
    out[t] = acc;
  }
}

// How many waves share one block of 32 owned rows (`row_blocks` of them) that streams `tiles`
// 32-row tiles of the other side: the number of splits and their length in rows.
// The planner's target (TFRS_SOFTMAX_WAVES), resolved once per entry-point call -- read per call: tests switch it --
// and handed down to every plan of that call.
static int64_t resolve_target_waves() {
  const char *v = option("TFRS_SOFTMAX_WAVES");
  return (v && *v) ? (int64_t)atoll(v) : (int64_t)2048;  // ~2 waves per SIMD on 256 CUs
}

static void softmax_plan_blocks(int64_t target_waves, int64_t row_blocks, int64_t tiles, int *nsplit,
                                int64_t *split_len) {
  int64_t want = (target_waves + row_blocks - 1) / row_blocks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t per = (tiles + want - 1) / want;
  *split_len = per * 32;
  *nsplit = (int)((tiles + per - 1) / per);
}

static int log2_padded_heads(int heads) {
  int lhp = 0;
  while ((1 << lhp) < heads) ++lhp;
  return lhp;
}

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

// The split plans of one problem and the workspace its loss kernels carve from the start of the buffer: the
// forward's pm, pl, ppos, the finalize kernel's block partials and its ticket; the backward's two partial-gradient
// buffers.  Waves own 32 / Hp queries in the forward / dq kernels (nsq splits of the candidates, lenq long) and 32
// candidates in the dc kernel (nsc splits of the flat query rows, lenc long).
struct SoftmaxLayout {
  int nsq, nsc;
  int64_t lenq, lenc;
  size_t fwd, bwd;
};

static SoftmaxLayout softmax_layout(int64_t nq, int heads, int64_t nc, int d) {
  SoftmaxLayout L;
  const int qw = 32 >> log2_padded_heads(heads);
  const int64_t target = resolve_target_waves();
  softmax_plan_blocks(target, (nq + qw - 1) / qw, (nc + 31) / 32, &L.nsq, &L.lenq);
  softmax_plan_blocks(target, (nc + 31) / 32, (nq + qw - 1) / qw, &L.nsc, &L.lenc);
  L.fwd = 2 * al((size_t)L.nsq * nq * 4) + al((size_t)nq * 4) + al((size_t)((nq + 255) / 256) * 8) + al(4);
  L.bwd = al((size_t)L.nsq * nq * heads * d * 4) + al((size_t)L.nsc * nc * d * 4);
  return L;
}

static SoftmaxArgs softmax_args(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                                const float *w, float inv_t, const float *corr, const int64_t *ids,
                                const uint8_t *mask) {
  SoftmaxArgs a = {};
  a.q = q; a.c = c; a.nq = nq; a.nc = nc; a.d = d;
  a.w = w; a.inv_t = inv_t; a.corr = corr; a.ids = ids; a.mask = mask;
  a.heads = heads; a.lhp = log2_padded_heads(heads);
  return a;
}

// f(std::integral_constant<int, DP>) for the padded dim the kernels are instantiated at
template <class F>
static void for_padded_dim(int d, F &&f) {
  switch (softmax_padded_dim(d)) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: f(std::integral_constant<int, 128>{}); break;
  }
}

// The loss forward on `a` (the SoftmaxArgs the launcher's kernel argument holds): sets the query plan, carves the
// workspace, launch(dp) runs the streaming kernel, then softmax_finalize_kernel on the partial (max, sum) pairs.
template <class Launch>
static int softmax_run_fwd(SoftmaxArgs &a, float *out_loss, float *out_lse, float *out_pos, void *workspace,
                           hipStream_t s, Launch &&launch) {
  const SoftmaxLayout L = softmax_layout(a.nq, a.heads, a.nc, a.d);
  a.nsplit = L.nsq; a.split_len = L.lenq;
  char *p = static_cast<char *>(workspace);
  a.pm = reinterpret_cast<float *>(p); p += al((size_t)L.nsq * a.nq * 4);
  a.pl = reinterpret_cast<float *>(p); p += al((size_t)L.nsq * a.nq * 4);
  a.ppos = reinterpret_cast<float *>(p); p += al((size_t)a.nq * 4);
  double *block_part = reinterpret_cast<double *>(p); p += al((size_t)((a.nq + 255) / 256) * 8);
  a.ticket = reinterpret_cast<uint32_t *>(p);
  for_padded_dim(a.d, launch);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(softmax_finalize_kernel, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, s, a, out_loss,
                     out_lse, out_pos, block_part, a.ticket);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// The loss backward on `a`: launch(dp, rows_are_queries) runs the gradient kernel on the plan and the partial
// buffer set here -- dq (waves own query blocks, stream candidates), then dc (waves own candidates, stream the flat
// (query, head) rows) -- and reduce_partials_kernel sums each one's nsplit partial buffers.
template <class Launch>
static int softmax_run_bwd(SoftmaxArgs &a, float *dq, float *dc, void *workspace, hipStream_t s, Launch &&launch) {
  const SoftmaxLayout L = softmax_layout(a.nq, a.heads, a.nc, a.d);
  auto reduce = [&](int64_t count, float *out) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)std::min<int64_t>((count + 255) / 256, 2048)),
                       dim3(256), 0, s, a.partial, a.nsplit, count, out);
  };
  char *p = static_cast<char *>(workspace);
  const int64_t nqd = a.nq * a.heads * a.d;
  a.nsplit = L.nsq; a.split_len = L.lenq;
  a.partial = reinterpret_cast<float *>(p);
  for_padded_dim(a.d, [&](auto dp) { launch(dp, std::true_type{}); });
  TFRS_LAUNCH_CHECK();
  reduce(nqd, dq);
  TFRS_LAUNCH_CHECK();
  p += al((size_t)L.nsq * nqd * 4);
  a.nsplit = L.nsc; a.split_len = L.lenc;
  a.partial = reinterpret_cast<float *>(p);
  for_padded_dim(a.d, [&](auto dp) { launch(dp, std::false_type{}); });
  TFRS_LAUNCH_CHECK();
  reduce(a.nc * a.d, dc);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

}  // namespace tfrs
