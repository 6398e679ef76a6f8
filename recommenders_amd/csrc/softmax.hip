// softmax.hip -- in-batch sampled-softmax loss of tfrs.tasks.Retrieval, forward and
// backward, without materialising the [nq, nc] logits; for 2-D queries q[nq, d] and for
// MULTI-HEAD (max-sim) queries q[nq, H, d], then also without the [nq*H, nc] head scores.
//
// Replaces (tasks/retrieval.py) the scores matmul :178-180 (multi-head: einsum "qne,ce->qnc" and
// reduce_max over heads :172-176), labels=eye :185, temperature
// :187-188, SamplingProbablityCorrection :190-192 (layers/loss.py:150-158),
// RemoveAccidentalHits :194-200 (layers/loss.py:114-147), score_mask :202-203 and the Keras
// CategoricalCrossentropy(from_logits, SUM) :210, plus their gradients
// (models/base.py:77).
//
//   M_bc  = max_h (q_bh . c_c)                 (the max is taken on the raw dot products; H = 1: q_b . c_c)
//   S_bc  = M_bc * inv_t - corr_c  [+ MIN_FLOAT if ids_c == ids_b, c != b]
//           [= MIN_FLOAT where !mask_bc]                                          (make_logit)
//   loss  = sum_b w_b (logsumexp_c S_bc - S_bb)
//   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) * inv_t      (0 where masked)
//   h*(b,c) = the LOWEST head index attaining the max (torch.max(dim) / first-index rule; TensorFlow's
//             reduce_max splits the gradient among tied heads instead)
//   dq_bh = sum_c [h == h*(b,c)] G_bc c_c ,   dc_c = sum_b G_bc q_{b,h*(b,c)}
//
// Structure (flash-attention like): a wave owns 32 rows of one side as the MFMA B operand
// and streams 32-row tiles of the other side as the A operand straight from L2 (both
// embedding matrices of a batch are a few MB).  Lanes index the owned rows, accumulator
// registers index the streamed rows, so the online max/sum of a row is lane-local.  In
// the backward the tile of G stays in the accumulator layout and is fed back as the B
// operand of the second GEMM (out^T[feature][row] += X^T G) -- no transposes.
// The streamed side is split across waves for occupancy; partial (max, sum) pairs and
// partial gradients are combined by small deterministic reduce kernels (no float atomics).
//
// Head layout (MH = true): the rows on the query side are the flat (query, head) rows with a query's
// heads ADJACENT: with Hp = the next power of two >= H a block of 32 rows holds 32 / Hp queries, head
// slot = row & (Hp - 1); slots H .. Hp-1 load zeros and enter the max as -inf.
//   forward, dq : the wave owns such a block, so a query's heads are lanes that differ in the low
//                 log2(Hp) bits of lane & 31: the head max of an accumulator register is log2(Hp)
//                 xor-exchanges, the lowest maximal head is the lowest set bit of the group's field of
//                 one ballot.  Every lane of a head group then carries the same online (m, l); head slot 0
//                 writes it.  dq multiplies G only into the winning head's lane.
//   dc          : the wave owns candidates and streams the flat rows, so a query's heads are accumulator
//                 registers: tile row (r & 3) + 8 (r >> 2) + 4 h.  Hp <= 4: register-local (r ^ 1, r ^ 2);
//                 Hp >= 8 adds one exchange with lane ^ 32, Hp = 16 / 32 the registers r ^ 4 / r ^ 8.
// MH = false is the same kernel at H = Hp = 1 with the head steps compiled out: the 2-D entry points.
//
// Roofline: MFMA-bound, 2*nq*nc*d flop forward and 8*nq*nc*d backward (S is recomputed
// once per gradient); at the MovieLens batch (4096 x 4096 x 64) the whole step is a few
// tens of microseconds, i.e. launch-latency territory.
#include "softmax_shared.h"

namespace tfrs {


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

// PLAIN: no sampling-probability correction, no accidental-hit removal, no score mask (the
// default Retrieval configuration): those branches are compiled out of the tile epilogue.
template <int DP, bool PLAIN, bool MH>
__global__ void __launch_bounds__(256) softmax_fwd_kernel(const SoftmaxArgs a_in) {
  SoftmaxArgs a = a_in;
  if (PLAIN) {
    a.corr = nullptr;
    a.ids = nullptr;
    a.mask = nullptr;
  }
  // re-arms the finalize kernel's ticket: it runs strictly after this kernel (a hipMemsetAsync
  // node is not reliably ordered against kernel nodes when the step replays from a HIP graph)
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.ticket = 0u;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lhp = MH ? a.lhp : 0, heads = MH ? a.heads : 1;
  const int hp = 1 << lhp, qw = 32 >> lhp;  // head slots per query, queries per wave
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  const int64_t nqb = (a.nq + qw - 1) / qw;
  if (wid >= nqb * a.nsplit) return;
  const int64_t qb = wid / a.nsplit;
  const int sp = (int)(wid - qb * a.nsplit);
  const int j = lane & 31, h = lane >> 5;
  const int hs = j & (hp - 1);
  const int64_t query = qb * qw + (j >> lhp);
  const bool qvalid = query < a.nq;
  const bool rvalid = qvalid && hs < heads;
  const bool vec_ok = (a.d == DP) && ((((uintptr_t)a.q) | ((uintptr_t)a.c)) % 16 == 0);

  float bq[DP / 2];
  load_row_frag<DP>(bq, a.q, query * heads + hs, rvalid, a.d, h, vec_ok);
  const int64_t id_q = (a.ids && qvalid) ? a.ids[query] : 0;

  float m = -__builtin_inff(), l = 0.0f, pos = 0.0f;
  bool haspos = false;
  const int64_t c_lo = (int64_t)sp * a.split_len;
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

    float s[16];
    float tmax = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float dot = acc[r];
      if constexpr (MH) dot = head_max_lanes<false>(rvalid ? acc[r] : -__builtin_inff(), hp, lane, hs, nullptr);
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
      l *= __expf(m - tmax);  // m = -inf on the first tile: exp(-inf) = 0, l = 0
      m = tmax;
    }
    if (m > -__builtin_inff()) {
#pragma unroll
      for (int r = 0; r < 16; ++r) l += __expf(s[r] - m);  // s = -inf contributes 0
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


// ROWS_ARE_QUERIES = true : wave owns 32 / Hp queries (32 flat rows), streams candidates, partial dq.
// ROWS_ARE_QUERIES = false: wave owns 32 candidates, streams the flat rows (slot space: query * Hp + head
//                           slot, a tile = 32 / Hp whole queries), partial dc.
template <int DP, bool ROWS_ARE_QUERIES, bool PLAIN, bool MH>
__global__ void __launch_bounds__(256) softmax_bwd_kernel(const SoftmaxArgs a_in) {
  SoftmaxArgs a = a_in;
  if (PLAIN) {
    a.corr = nullptr;
    a.ids = nullptr;
    a.mask = nullptr;
  }
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
  if (rvalid) {
    if (ROWS_ARE_QUERIES) {
      lse_r = a.lse[q_own];
      if (a.w) w_r = a.w[q_own];
      if (a.ids) id_r = a.ids[q_own];  // nq <= nc, so a query is also a valid candidate row
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
    *row = (u >> lhp) * heads + hs;
    return u < n_s && hs < heads;
  };
  const float *sdata = ROWS_ARE_QUERIES ? a.c : a.q;

  // Streamed tile (32 rows x DP features): fetched one tile ahead into registers (row j, half h
  // = the first GEMM's A fragment) and mirrored into this wave's LDS slab so that the second
  // GEMM can read it transposed (lane = feature) with conflict-free ds_read_b32.
  constexpr int kLd = DP + 4;  // floats per LDS row (+16 B: rows start in different bank groups)
  extern __shared__ __attribute__((aligned(16))) float smem_sm[];
  float *slab = smem_sm + (size_t)wave * 32 * kLd;
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
        const float v = make_logit(best[r], query, cand, a, corr_c, id_q, id_c, &masked);
        const float lse_q = ROWS_ARE_QUERIES ? lse_r : a.lse[query];
        const float w_q = ROWS_ARE_QUERIES ? w_r : (a.w ? a.w[query] : 1.0f);
        const float p = __expf(v - lse_q);
        gg = masked ? 0.0f : w_q * (p - (cand == query ? 1.0f : 0.0f)) * gl;
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


template <int DP, bool MH>
static void launch_fwd(const SoftmaxArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t waves = ((a.nq + qw - 1) / qw) * a.nsplit;
  if (!a.corr && !a.ids && !a.mask)
    hipLaunchKernelGGL((softmax_fwd_kernel<DP, true, MH>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((softmax_fwd_kernel<DP, false, MH>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
}

template <int DP, bool RQ, bool MH>
static void launch_bwd(const SoftmaxArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t blocks = RQ ? (a.nq + qw - 1) / qw : (a.nc + 31) / 32;
  const int64_t waves = blocks * a.nsplit;
  const size_t lds = (size_t)4 * 32 * (DP + 4) * sizeof(float);
  if (!a.corr && !a.ids && !a.mask)
    hipLaunchKernelGGL((softmax_bwd_kernel<DP, RQ, true, MH>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((softmax_bwd_kernel<DP, RQ, false, MH>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, s, a);
}

// workspace of the f32 kernels: the forward's partials or the backward's two partial-gradient buffers
static size_t f32_workspace_bytes(int64_t nq, int heads, int64_t nc, int d) {
  const int lhp = log2_padded_heads(heads);
  int nsq, nsc;
  int64_t len;
  const int64_t target = resolve_target_waves();
  plan_queries(target, nq, lhp, nc, &nsq, &len);
  plan_candidates(target, nq, lhp, nc, &nsc, &len);
  const size_t fwd = 2 * al((size_t)nsq * nq * 4) + al((size_t)nq * 4) +
                     al((size_t)((nq + 255) / 256) * 8) + al(4);  // + finalize partials, ticket
  const size_t bwd = al((size_t)nsq * nq * heads * d * 4) + al((size_t)nsc * nc * d * 4);
  return fwd > bwd ? fwd : bwd;
}

static SoftmaxArgs make_args(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                             const float *w, float inv_t, const float *corr, const int64_t *ids,
                             const uint8_t *mask) {
  SoftmaxArgs a = {};
  a.q = q; a.c = c; a.nq = nq; a.nc = nc; a.d = d;
  a.w = w; a.inv_t = inv_t; a.corr = corr; a.ids = ids; a.mask = mask;
  a.heads = heads; a.lhp = log2_padded_heads(heads);
  return a;
}

// forward kernel + finalize; carves pm, pl, ppos, the finalize partials and the ticket out of the workspace
template <bool MH>
static int run_fwd(SoftmaxArgs a, float *out_loss, float *out_lse, float *out_pos, void *workspace,
                   hipStream_t s) {
  plan_queries(resolve_target_waves(), a.nq, a.lhp, a.nc, &a.nsplit, &a.split_len);
  char *p = static_cast<char *>(workspace);
  a.pm = reinterpret_cast<float *>(p); p += al((size_t)a.nsplit * a.nq * 4);
  a.pl = reinterpret_cast<float *>(p); p += al((size_t)a.nsplit * a.nq * 4);
  a.ppos = reinterpret_cast<float *>(p); p += al((size_t)a.nq * 4);
  double *block_part = reinterpret_cast<double *>(p); p += al((size_t)((a.nq + 255) / 256) * 8);
  a.ticket = reinterpret_cast<uint32_t *>(p);
  for_padded_dim(a.d, [&](auto dp) { launch_fwd<decltype(dp)::value, MH>(a, s); });
  TFRS_LAUNCH_CHECK();
  softmax_launch_finalize(a, out_loss, out_lse, out_pos, block_part, s);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

template <bool MH>
static int run_bwd(SoftmaxArgs a, float *dq, float *dc, void *workspace, hipStream_t s) {
  char *p = static_cast<char *>(workspace);
  const int64_t target = resolve_target_waves();

  // dq: waves own query blocks, stream candidates
  plan_queries(target, a.nq, a.lhp, a.nc, &a.nsplit, &a.split_len);
  a.partial = reinterpret_cast<float *>(p);
  const int64_t nqd = a.nq * a.heads * a.d;
  for_padded_dim(a.d, [&](auto dp) { launch_bwd<decltype(dp)::value, true, MH>(a, s); });
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.partial, a.nsplit, nqd, dq, s);
  TFRS_LAUNCH_CHECK();

  // dc: waves own candidates, stream the flat (query, head) rows
  p += al((size_t)a.nsplit * nqd * 4);
  plan_candidates(target, a.nq, a.lhp, a.nc, &a.nsplit, &a.split_len);
  a.partial = reinterpret_cast<float *>(p);
  for_padded_dim(a.d, [&](auto dp) { launch_bwd<decltype(dp)::value, false, MH>(a, s); });
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.partial, a.nsplit, a.nc * a.d, dc, s);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// softmax16.hip: the split-fp16 path
size_t softmax16_workspace_bytes(int64_t nq, int64_t nc, int d);
int softmax16_forward(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w,
                      float inv_t, float *out_loss, float *out_lse, float *out_pos, void *ws,
                      hipStream_t s);
int softmax16_backward(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w,
                       float inv_t, const float *lse, const float *gloss, float *dq, float *dc,
                       void *ws, int reuse, hipStream_t s);

// TFRS_SOFTMAX_MODE=f32 keeps everything on the f32-MFMA kernels; default: the split-fp16 path
// whenever no logit option that needs per-element side inputs is set.
static bool use_f16_path(const float *corr, const int64_t *ids, const uint8_t *mask) {
  const char *v = option("TFRS_SOFTMAX_MODE");   // read per call: tests switch it
  const bool f32_only = v && v[0] == 'f' && v[1] == '3';
  return !f32_only && !corr && !ids && !mask;
}

}  // namespace tfrs

using namespace tfrs;

// ---- 2-D queries: the MH = false kernels, or the split-fp16 path
static int check_common(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                        const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1 && d >= 1, "%s: bad shape", who);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  if (d > 128) {
    set_error("%s: embedding dim %d > 128 is not implemented", who, d);
    return TFRS_ENOTIMPL;
  }
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_softmax_workspace_bytes(int64_t nq, int64_t nc, int d) {
  if (nq < 1 || nc < 1 || d < 1) return 256;
  const size_t f32 = f32_workspace_bytes(nq, 1, nc, d);
  const size_t f16 = d <= 128 ? softmax16_workspace_bytes(nq, nc, d) : 0;
  return f32 > f16 ? f32 : f16;
}

extern "C" int tfrs_inbatch_softmax_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                           int d, const float *sample_weight,
                                           float inv_temperature, const float *log_q_correction,
                                           const int64_t *cand_ids, const uint8_t *score_mask,
                                           float *out_loss, float *out_lse, float *out_pos,
                                           void *workspace, size_t workspace_bytes, void *stream) {
  int rc = check_common(q, c, nq, nc, d, "inbatch_softmax_ce_fwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos && workspace, "inbatch_softmax_ce_fwd: NULL output");
  if (workspace_bytes < tfrs_inbatch_softmax_workspace_bytes(nq, nc, d)) {
    set_error("inbatch_softmax_ce_fwd: workspace too small");
    return TFRS_ENOMEM;
  }
  if (use_f16_path(log_q_correction, cand_ids, score_mask))
    return softmax16_forward(q, c, nq, nc, d, sample_weight, inv_temperature, out_loss, out_lse,
                             out_pos, workspace, (hipStream_t)stream);
  return run_fwd<false>(make_args(q, c, nq, 1, nc, d, sample_weight, inv_temperature, log_q_correction,
                                  cand_ids, score_mask),
                        out_loss, out_lse, out_pos, workspace, (hipStream_t)stream);
}

extern "C" int tfrs_inbatch_softmax_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                           int d, const float *sample_weight,
                                           float inv_temperature, const float *log_q_correction,
                                           const int64_t *cand_ids, const uint8_t *score_mask,
                                           const float *lse, const float *gloss, float *dq,
                                           float *dc, void *workspace, size_t workspace_bytes,
                                           int reuse_forward_workspace, void *stream) {
  int rc = check_common(q, c, nq, nc, d, "inbatch_softmax_ce_bwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(lse && dq && dc && workspace, "inbatch_softmax_ce_bwd: NULL pointer");
  if (workspace_bytes < tfrs_inbatch_softmax_workspace_bytes(nq, nc, d)) {
    set_error("inbatch_softmax_ce_bwd: workspace too small");
    return TFRS_ENOMEM;
  }
  if (use_f16_path(log_q_correction, cand_ids, score_mask))
    return softmax16_backward(q, c, nq, nc, d, sample_weight, inv_temperature, lse, gloss, dq, dc,
                              workspace, reuse_forward_workspace, (hipStream_t)stream);
  SoftmaxArgs a = make_args(q, c, nq, 1, nc, d, sample_weight, inv_temperature, log_q_correction, cand_ids,
                            score_mask);
  a.lse = lse; a.gloss = gloss;
  return run_bwd<false>(a, dq, dc, workspace, (hipStream_t)stream);
}

// The split geometry of the f32 kernels under the options in force (host only, no device call): nsplit and split_len
// of plan_queries (forward, dq) and of plan_candidates (dc), from the planners the launches above use.
extern "C" int tfrs_inbatch_softmax_plan_f32(int64_t nq, int heads, int64_t nc, int64_t *out) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= nq && heads >= 1 && heads <= 32 && out, "inbatch_softmax_plan_f32: bad argument");
  const int lhp = log2_padded_heads(heads);
  const int64_t target = resolve_target_waves();
  int ns;
  plan_queries(target, nq, lhp, nc, &ns, &out[1]);
  out[0] = ns;
  plan_candidates(target, nq, lhp, nc, &ns, &out[3]);
  out[2] = ns;
  return TFRS_OK;
}

// ---- multi-head queries: the MH = true kernels for every heads in 1 .. 32
static int check_common_mh(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                           const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1, "%s: bad shape (nq=%lld, nc=%lld)", who, (long long)nq, (long long)nc);
  TFRS_CHECK_ARG(heads >= 1 && heads <= 32, "%s: heads=%d outside [1, 32]", who, heads);
  TFRS_CHECK_ARG(d >= 1 && d <= TFRS_MAX_DIM, "%s: embedding dim=%d outside [1, %d]", who, d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_softmax_mh_workspace_bytes(int64_t nq, int heads, int64_t nc, int d) {
  if (nq < 1 || nc < 1 || d < 1 || heads < 1 || heads > 32) return 256;
  return f32_workspace_bytes(nq, heads, nc, d);
}

extern "C" int tfrs_inbatch_softmax_mh_ce_fwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, float *out_loss, float *out_lse,
                                              float *out_pos, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common_mh(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_fwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos && workspace, "inbatch_softmax_mh_ce_fwd: NULL output");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_fwd: workspace too small");
  return run_fwd<true>(make_args(q, c, nq, heads, nc, d, sample_weight, inv_temperature, log_q_correction,
                                 cand_ids, score_mask),
                       out_loss, out_lse, out_pos, workspace, (hipStream_t)stream);
}

extern "C" int tfrs_inbatch_softmax_mh_ce_bwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, const float *lse, const float *gloss,
                                              float *dq, float *dc, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common_mh(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_bwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(lse && dq && dc && workspace, "inbatch_softmax_mh_ce_bwd: NULL pointer");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_bwd: workspace too small");
  SoftmaxArgs a = make_args(q, c, nq, heads, nc, d, sample_weight, inv_temperature, log_q_correction, cand_ids,
                            score_mask);
  a.lse = lse; a.gloss = gloss;
  return run_bwd<true>(a, dq, dc, workspace, (hipStream_t)stream);
}
