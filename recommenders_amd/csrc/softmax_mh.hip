// softmax_mh.hip -- the in-batch sampled-softmax loss of tfrs.tasks.Retrieval for MULTI-HEAD
// (max-sim) queries q[nq, H, d], forward and backward, without the [nq*H, nc] head scores or
// the [nq, nc] logits (tasks/retrieval.py:172-176: einsum "qne,ce->qnc", reduce_max over heads).
//
//   M_bc  = max_h (q_bh . c_c)                 (the max is taken on the raw dot products)
//   S_bc  = make_logit(M_bc)                   (inv_t, - correction, accidental hits, mask: softmax_args.h)
//   loss  = sum_b w_b (logsumexp_c S_bc - S_bb)
//   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) * inv_t      (0 where masked)
//   h*(b,c) = the LOWEST head index attaining the max (torch.max(dim) / first-index rule; TensorFlow's
//             reduce_max splits the gradient among tied heads instead)
//   dq_bh = sum_c [h == h*(b,c)] G_bc c_c ,   dc_c = sum_b G_bc q_{b,h*(b,c)}
//
// Structure: softmax.hip's.  A wave owns 32 rows of one side as the MFMA B operand and streams 32-row
// tiles of the other side; lanes index the owned rows, the 16 accumulator registers (and the lane half)
// index the streamed rows; partial (max, sum) pairs and partial gradients of the splits of the streamed
// side go through softmax.hip's finalize / reduce kernels.  No float atomics, no score buffer.
//
// The rows on the query side are the flat (query, head) rows with a query's heads ADJACENT: with
// Hp = the next power of two >= H a block of 32 rows holds 32 / Hp queries, head slot = row & (Hp - 1);
// slots H .. Hp-1 load zeros and enter the max as -inf.
//   forward, dq : the wave owns such a block, so a query's heads are lanes that differ in the low
//                 log2(Hp) bits of lane & 31: the head max of an accumulator register is log2(Hp)
//                 xor-exchanges, the lowest maximal head is the lowest set bit of the group's field of
//                 one ballot.  Every lane of a head group then carries the same online (m, l); head slot 0
//                 writes it.  dq multiplies G only into the winning head's lane.
//   dc          : the wave owns candidates and streams the flat rows, so a query's heads are accumulator
//                 registers: tile row (r & 3) + 8 (r >> 2) + 4 h.  Hp <= 4: register-local (r ^ 1, r ^ 2);
//                 Hp >= 8 adds one exchange with lane ^ 32, Hp = 16 / 32 the registers r ^ 4 / r ^ 8.
#include <algorithm>

#include "softmax_args.h"

namespace tfrs {

struct MhArgs : SoftmaxArgs {
  int heads;  // H
  int lhp;    // log2(Hp)
};

template <int DP, bool PLAIN>
__global__ void __launch_bounds__(256) softmax_mh_fwd_kernel(const MhArgs a_in) {
  MhArgs a = a_in;
  if (PLAIN) {
    a.corr = nullptr;
    a.ids = nullptr;
    a.mask = nullptr;
  }
  // re-arms the finalize kernel's ticket, as softmax_fwd_kernel does (graph replay)
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.ticket = 0u;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hp = 1 << a.lhp, qw = 32 >> a.lhp;  // head slots per query, queries per wave
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  const int64_t nqb = (a.nq + qw - 1) / qw;
  if (wid >= nqb * a.nsplit) return;
  const int64_t qb = wid / a.nsplit;
  const int sp = (int)(wid - qb * a.nsplit);
  const int j = lane & 31, h = lane >> 5;
  const int hs = j & (hp - 1);
  const int64_t query = qb * qw + (j >> a.lhp);
  const bool qvalid = query < a.nq;
  const bool rvalid = qvalid && hs < a.heads;
  const bool vec_ok = (a.d == DP) && ((((uintptr_t)a.q) | ((uintptr_t)a.c)) % 16 == 0);

  float bq[DP / 2];
  load_row_frag<DP>(bq, a.q, query * a.heads + hs, rvalid, a.d, h, vec_ok);
  const int64_t id_q = (a.ids && qvalid) ? a.ids[query] : 0;

  float m = -__builtin_inff(), l = 0.0f, pos = 0.0f;
  bool haspos = false;
  const int64_t c_lo = (int64_t)sp * a.split_len;
  int64_t c_hi = c_lo + a.split_len;
  if (c_hi > a.nc) c_hi = a.nc;

  float af_next[DP / 2];
  load_row_frag<DP>(af_next, a.c, c_lo + j, c_lo + j < a.nc && c_lo < c_hi, a.d, h, vec_ok);
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) af[s] = af_next[s];
    if (c0 + 32 < c_hi) load_row_frag<DP>(af_next, a.c, c0 + 32 + j, c0 + 32 + j < a.nc, a.d, h, vec_ok);
    const f32x16 acc = tile_dot<DP>(af, bq);

    float s[16];
    float tmax = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // head max: every lane of the query's group ends with the same value (all lanes take part)
      float dot = rvalid ? acc[r] : -__builtin_inff();
      for (int x = 1; x < hp; x <<= 1) dot = fmaxf(dot, __shfl_xor(dot, x));
      const int64_t cand = c0 + tile_row_of_reg(r, h);
      float v = -__builtin_inff();
      if (qvalid && cand < c_hi) {
        bool masked;
        v = make_logit(dot, query, cand, a, a.corr ? a.corr[cand] : 0.0f, id_q,
                       a.ids ? a.ids[cand] : 0, &masked);
        if (cand == query) {
          pos = v;
          haspos = true;
        }
      }
      s[r] = v;
      tmax = fmaxf(tmax, v);
    }
    if (tmax > m) {
      l *= __expf(m - tmax);
      m = tmax;
    }
    if (m > -__builtin_inff()) {
#pragma unroll
      for (int r = 0; r < 16; ++r) l += __expf(s[r] - m);
    }
  }

  // the two lane halves hold disjoint candidates of the same query
  const float m2 = __shfl_xor(m, 32), l2 = __shfl_xor(l, 32);
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (m > -__builtin_inff()) ll += l * __expf(m - mm);
  if (m2 > -__builtin_inff()) ll += l2 * __expf(m2 - mm);
  if (h == 0 && hs == 0 && qvalid) {
    a.pm[(int64_t)sp * a.nq + query] = mm;
    a.pl[(int64_t)sp * a.nq + query] = ll;
  }
  if (haspos && hs == 0) a.ppos[query] = pos;  // one lane of one split: head slot 0 of the half that sees c == b
}

// (v2, i2) beats (v1, i1): larger value, or the same value at a lower head index
__device__ __forceinline__ void take_better(float &v1, int &i1, float v2, int i2) {
  const bool t = v2 > v1 || (v2 == v1 && i2 < i1);
  v1 = t ? v2 : v1;
  i1 = t ? i2 : i1;
}

// ROWS_ARE_QUERIES = true : wave owns 32 / Hp queries (32 flat rows), streams candidates, partial dq.
// ROWS_ARE_QUERIES = false: wave owns 32 candidates, streams the flat rows (slot space: query * Hp + head
//                           slot, a tile = 32 / Hp whole queries), partial dc.
template <int DP, bool ROWS_ARE_QUERIES, bool PLAIN>
__global__ void __launch_bounds__(256) softmax_mh_bwd_kernel(const MhArgs a_in) {
  MhArgs a = a_in;
  if (PLAIN) {
    a.corr = nullptr;
    a.ids = nullptr;
    a.mask = nullptr;
  }
  constexpr int NFB = (DP + 31) / 32;  // 32-feature output blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lhp = a.lhp, hp = 1 << lhp, qw = 32 >> lhp;
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
  const int64_t rrow = ROWS_ARE_QUERIES ? q_own * a.heads + hs_own : rb * 32 + j;  // row of q / of c, and of the output
  const bool rvalid = ROWS_ARE_QUERIES ? (q_own < a.nq && hs_own < a.heads) : (rrow < a.nc);

  float br[DP / 2];
  load_row_frag<DP>(br, ROWS_ARE_QUERIES ? a.q : a.c, rrow, rvalid, a.d, h, vec_ok);

  float lse_r = 0.0f, w_r = 1.0f, corr_r = 0.0f;
  int64_t id_r = 0;
  if (rvalid) {
    if (ROWS_ARE_QUERIES) {
      lse_r = a.lse[q_own];
      if (a.w) w_r = a.w[q_own];
      if (a.ids) id_r = a.ids[q_own];  // nq <= nc
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

  // streamed row of lane j in the tile at s0: candidate s0 + j, or the flat row of slot s0 + j
  auto stream_row = [&](int64_t u, int64_t *row) -> bool {
    if (ROWS_ARE_QUERIES) {
      *row = u;
      return u < n_s;
    }
    const int hs = (int)(u & (hp - 1));
    *row = (u >> lhp) * a.heads + hs;
    return u < n_s && hs < a.heads;
  };
  const float *sdata = ROWS_ARE_QUERIES ? a.c : a.q;

  constexpr int kLd = DP + 4;  // floats per LDS row (+16 B: rows start in different bank groups)
  extern __shared__ __attribute__((aligned(16))) float smem_mh[];
  float *slab = smem_mh + (size_t)wave * 32 * kLd;
  float af_next[DP / 2];
  {
    int64_t row;
    const bool ok = stream_row(s_lo + j, &row);
    load_row_frag<DP>(af_next, sdata, row, ok && s_lo < s_hi, a.d, h, vec_ok);
  }

  for (int64_t s0 = s_lo; s0 < s_hi; s0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) af[s] = af_next[s];
    if (s0 + 32 < s_hi) {
      int64_t row;
      const bool ok = stream_row(s0 + 32 + j, &row);
      load_row_frag<DP>(af_next, sdata, row, ok, a.d, h, vec_ok);
    }
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
    if (ROWS_ARE_QUERIES) {
      const uint32_t field = hp == 32 ? 0xFFFFFFFFu : ((1u << hp) - 1u);
      const int shift = h * 32 + (j & ~(hp - 1));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float own = rvalid ? acc[r] : -__builtin_inff();
        float v = own;
        for (int x = 1; x < hp; x <<= 1) v = fmaxf(v, __shfl_xor(v, x));
        const uint64_t tied = __ballot(own == v);
        const uint32_t grp = (uint32_t)(tied >> shift) & field;   // bit s: head slot s attains the max
        best[r] = v;
        win[r] = rvalid && s0 + tile_row_of_reg(r, h) < s_hi && (grp & (0u - grp)) == (1u << hs_own);
      }
    } else {
      int bi[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tile_row_of_reg(r, h);
        const int hs = t & (hp - 1);
        const bool valid = rvalid && s0 + t < s_hi && hs < a.heads;
        best[r] = valid ? acc[r] : -__builtin_inff();
        bi[r] = hs;
      }
      if (lhp >= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(r & 1)) {
            take_better(best[r], bi[r], best[r | 1], bi[r | 1]);
            best[r | 1] = best[r];
            bi[r | 1] = bi[r];
          }
      }
      if (lhp >= 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(r & 2)) {
            take_better(best[r], bi[r], best[r | 2], bi[r | 2]);
            best[r | 2] = best[r];
            bi[r | 2] = bi[r];
          }
      }
      if (lhp >= 3) {  // tile rows t and t ^ 4 are the two lane halves
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ov = __shfl_xor(best[r], 32);
          const int oi = __shfl_xor(bi[r], 32);
          take_better(best[r], bi[r], ov, oi);
        }
      }
      if (lhp >= 4) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(r & 4)) {
            take_better(best[r], bi[r], best[r | 4], bi[r | 4]);
            best[r | 4] = best[r];
            bi[r | 4] = bi[r];
          }
      }
      if (lhp >= 5) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(r & 8)) {
            take_better(best[r], bi[r], best[r | 8], bi[r | 8]);
            best[r | 8] = best[r];
            bi[r | 8] = bi[r];
          }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = tile_row_of_reg(r, h);
        const int hs = t & (hp - 1);
        win[r] = rvalid && s0 + t < s_hi && hs < a.heads && bi[r] == hs;
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
        const float v = make_logit(best[r], query, cand, a, corr_c, id_q, id_c, &masked);
        const float lse_q = ROWS_ARE_QUERIES ? lse_r : a.lse[query];
        const float w_q = ROWS_ARE_QUERIES ? w_r : (a.w ? a.w[query] : 1.0f);
        const float p = __expf(v - lse_q);
        gg = masked ? 0.0f : w_q * (p - (cand == query ? 1.0f : 0.0f)) * gl;
      }
      g[r] = gg;
    }

    // out^T[feature][owned row] += sum over the 32 streamed rows of X[srow][feature] * G[srow][row]
    // (softmax_bwd_kernel's second GEMM: G stays in the accumulator layout, X is read from the slab)
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
    const int64_t n_out = ROWS_ARE_QUERIES ? a.nq * a.heads : a.nc;
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

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

static int log2_padded_heads(int heads) {
  int lhp = 0;
  while ((1 << lhp) < heads) ++lhp;
  return lhp;
}

// splits of the forward / dq kernels (waves own query blocks) and of the dc kernel (waves own candidates)
static void plan_queries(int64_t nq, int lhp, int64_t nc, int *nsplit, int64_t *split_len) {
  const int qw = 32 >> lhp;
  softmax_plan_blocks((nq + qw - 1) / qw, (nc + 31) / 32, nsplit, split_len);
}
static void plan_candidates(int64_t nq, int lhp, int64_t nc, int *nsplit, int64_t *split_len) {
  const int qw = 32 >> lhp;
  softmax_plan_blocks((nc + 31) / 32, (nq + qw - 1) / qw, nsplit, split_len);
}

template <int DP>
static void launch_fwd(const MhArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t waves = ((a.nq + qw - 1) / qw) * a.nsplit;
  if (!a.corr && !a.ids && !a.mask)
    hipLaunchKernelGGL((softmax_mh_fwd_kernel<DP, true>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((softmax_mh_fwd_kernel<DP, false>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
}

template <int DP, bool RQ>
static void launch_bwd(const MhArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t blocks = RQ ? (a.nq + qw - 1) / qw : (a.nc + 31) / 32;
  const int64_t waves = blocks * a.nsplit;
  const size_t lds = (size_t)4 * 32 * (DP + 4) * sizeof(float);
  if (!a.corr && !a.ids && !a.mask)
    hipLaunchKernelGGL((softmax_mh_bwd_kernel<DP, RQ, true>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((softmax_mh_bwd_kernel<DP, RQ, false>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, s, a);
}

}  // namespace tfrs

using namespace tfrs;

static int check_common(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d, const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1, "%s: bad shape (nq=%lld, nc=%lld)", who, (long long)nq, (long long)nc);
  TFRS_CHECK_ARG(heads >= 1 && heads <= 32, "%s: heads=%d outside [1, 32]", who, heads);
  TFRS_CHECK_ARG(d >= 1 && d <= TFRS_MAX_DIM, "%s: embedding dim=%d outside [1, %d]", who, d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_softmax_mh_workspace_bytes(int64_t nq, int heads, int64_t nc, int d) {
  if (nq < 1 || nc < 1 || d < 1 || heads < 1 || heads > 32) return 256;
  const int lhp = log2_padded_heads(heads);
  int nsq, nsc;
  int64_t len;
  plan_queries(nq, lhp, nc, &nsq, &len);
  plan_candidates(nq, lhp, nc, &nsc, &len);
  const size_t fwd = 2 * al((size_t)nsq * nq * 4) + al((size_t)nq * 4) +
                     al((size_t)((nq + 255) / 256) * 8) + al(4);  // + finalize partials, ticket
  const size_t bwd = al((size_t)nsq * nq * heads * d * 4) + al((size_t)nsc * nc * d * 4);
  return fwd > bwd ? fwd : bwd;
}

extern "C" int tfrs_inbatch_softmax_mh_ce_fwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, float *out_loss, float *out_lse,
                                              float *out_pos, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_fwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos && workspace, "inbatch_softmax_mh_ce_fwd: NULL output");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_fwd: workspace too small");
  MhArgs a = {};
  a.q = q; a.c = c; a.nq = nq; a.nc = nc; a.d = d;
  a.w = sample_weight; a.inv_t = inv_temperature; a.corr = log_q_correction;
  a.ids = cand_ids; a.mask = score_mask;
  a.heads = heads; a.lhp = log2_padded_heads(heads);
  plan_queries(nq, a.lhp, nc, &a.nsplit, &a.split_len);
  char *p = static_cast<char *>(workspace);
  a.pm = reinterpret_cast<float *>(p); p += al((size_t)a.nsplit * nq * 4);
  a.pl = reinterpret_cast<float *>(p); p += al((size_t)a.nsplit * nq * 4);
  a.ppos = reinterpret_cast<float *>(p); p += al((size_t)nq * 4);
  double *block_part = reinterpret_cast<double *>(p); p += al((size_t)((nq + 255) / 256) * 8);
  a.ticket = reinterpret_cast<uint32_t *>(p);
  hipStream_t s = (hipStream_t)stream;
  switch (softmax_padded_dim(d)) {
    case 8: launch_fwd<8>(a, s); break;
    case 16: launch_fwd<16>(a, s); break;
    case 32: launch_fwd<32>(a, s); break;
    case 64: launch_fwd<64>(a, s); break;
    default: launch_fwd<128>(a, s); break;
  }
  TFRS_LAUNCH_CHECK();
  softmax_launch_finalize(a, out_loss, out_lse, out_pos, block_part, s);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_softmax_mh_ce_bwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, const float *lse, const float *gloss,
                                              float *dq, float *dc, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_bwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(lse && dq && dc && workspace, "inbatch_softmax_mh_ce_bwd: NULL pointer");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  MhArgs a = {};
  a.q = q; a.c = c; a.nq = nq; a.nc = nc; a.d = d;
  a.w = sample_weight; a.inv_t = inv_temperature; a.corr = log_q_correction;
  a.ids = cand_ids; a.mask = score_mask; a.lse = lse; a.gloss = gloss;
  a.heads = heads; a.lhp = log2_padded_heads(heads);
  char *p = static_cast<char *>(workspace);

  // dq: waves own query blocks, stream candidates
  plan_queries(nq, a.lhp, nc, &a.nsplit, &a.split_len);
  a.partial = reinterpret_cast<float *>(p);
  const int nsq = a.nsplit;
  switch (softmax_padded_dim(d)) {
    case 8: launch_bwd<8, true>(a, s); break;
    case 16: launch_bwd<16, true>(a, s); break;
    case 32: launch_bwd<32, true>(a, s); break;
    case 64: launch_bwd<64, true>(a, s); break;
    default: launch_bwd<128, true>(a, s); break;
  }
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.partial, nsq, nq * heads * d, dq, s);
  TFRS_LAUNCH_CHECK();

  // dc: waves own candidates, stream the flat (query, head) rows
  p += al((size_t)nsq * nq * heads * d * 4);
  plan_candidates(nq, a.lhp, nc, &a.nsplit, &a.split_len);
  a.partial = reinterpret_cast<float *>(p);
  switch (softmax_padded_dim(d)) {
    case 8: launch_bwd<8, false>(a, s); break;
    case 16: launch_bwd<16, false>(a, s); break;
    case 32: launch_bwd<32, false>(a, s); break;
    case 64: launch_bwd<64, false>(a, s); break;
    default: launch_bwd<128, false>(a, s); break;
  }
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.partial, a.nsplit, nc * d, dc, s);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
