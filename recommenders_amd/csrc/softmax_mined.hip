// softmax_mined.hip -- hard-negative mining, the softmax cross-entropy on the mined logits and the batch metric's
// rank count, all over ADJUSTED in-batch logits and without the [nq, nc] matrix (2-D queries).
//
// Replaces (tasks/retrieval.py) :178-203 (scores, temperature, SamplingProbablityCorrection,
// RemoveAccidentalHits, score_mask), HardNegativeMining :205-208 (layers/loss.py:91-109), the cross-entropy :210
// on the mined logits and in_top_k of the batch metrics :228-232.
//
//   S_bc  = (q_b . c_c) / T - corr_c  [+ MIN_FLOAT if ids_c == ids_b, c != b]  [= MIN_FLOAT where !mask_bc]
//           (IEEE f32 division, as the reference's scores / temperature; -0 -> +0)            (mined_logit)
//   keep(b, c) = (c == b) || S_bc > tau_b || (S_bc == tau_b && c <= cut_b)
//   tau_b = the n-th largest negative logit of row b, cut_b = the column of the last tied negative taken
//           (INT64_MAX: every tie at tau_b is taken) -- top_k's lower-column-first rule
//   loss  = sum_b w_b (logsumexp_{c : keep} S_bc - S_bb)
//   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) / T   where keep(b, c) and not masked, else 0
//   count_b = #{c != b : keep(b, c) and S_bc > S_bb}
//
// Every kernel is the tile loop of softmax.hip: a wave owns 32 rows as the MFMA B operand and streams 32-row
// tiles of the other side; a logit exists only in an accumulator register.  keep() compares RECOMPUTED logits
// with tau for equality, so every kernel forms S_bc by the same tile_dot over the same fragments (the dc
// kernel swaps the operand roles: each product commutes and the k order is the same) and the same mined_logit.
//
// Selection (exact, fixed launch sequence, no host read-back, no float atomics): a radix select over the
// order-preserving uint32 image of S (f32_orderable), four 8-bit passes.  A pass re-scores the tiles; every
// negative whose key matches the prefix fixed so far bumps hist[row][digit] in LDS (row stride 257 words:
// equal digits of different rows fall into different banks -- in the first pass nearly all digits are equal),
// the non-zero bins are flushed with integer atomicAdd into hist[nq, 256].  mined_pick_kernel then walks a
// row's bins from the top, fixes the digit, lowers the remaining rank and zeroes the bins for the next pass.
// After pass four a row knows tau, how many ties exist and how many it takes.  Only a row that takes FEWER
// ties than exist needs a cut column (real inputs do that: every masked / accidental-hit logit is exactly
// MIN_FLOAT): one scoring pass stores per-(split, row) tie counts, one more finds the r-th tie in column order
// in the split that holds it.  Both exit wave-uniformly when no row of the wave needs a cut.
#include "softmax_shared.h"

namespace tfrs {

constexpr int kHistStride = 257;   // words per row of the LDS histogram
constexpr int64_t kCutAll = INT64_MAX;

struct MinedArgs {
  SoftmaxArgs s;         // operands, options, split plan, partial buffers; s.inv_t = 1 / t is the gradient factor only
  float t;               // the temperature: divides the dot product
  const float *tau;      // [nq] threshold per row, or NULL: keep everything
  const int64_t *cut;    // [nq] cut column per row (read only with tau)
  // selection state (workspace)
  uint32_t *hist;        // [nq, 256] bins of the current pass
  uint32_t *prefix;      // [nq] key bits fixed so far
  uint32_t *krem;        // [nq] rank still wanted among the keys that match the prefix; after pass four: ties taken
  uint32_t *need;        // [nq] 1: the row takes fewer ties than exist
  uint32_t *tiecnt;      // [nsplit, nq] ties per split
  float *tau_w;          // [nq] outputs of the selection
  int64_t *cut_w;
  int pass;              // 0 .. 3
  uint32_t *cnt_part;    // [nsplit, nq] rank-count partials
};

enum { kModeHist = 0, kModeTieCount = 1, kModeTieFind = 2, kModeFwd = 3, kModeCount = 4 };

__device__ __forceinline__ float mined_logit(float dot, int64_t query, int64_t cand, const MinedArgs &a,
                                             float corr_c, int64_t id_q, int64_t id_c, bool *masked) {
  float v = __fdiv_rn(dot, a.t);
  if (a.s.corr) v -= corr_c;
  if (a.s.ids && cand != query && id_c == id_q) v += kMinFloat;
  *masked = false;
  if (a.s.mask && !a.s.mask[query * a.s.nc + cand]) {
    v = kMinFloat;
    *masked = true;
  }
  return v + 0.0f;  // -0 -> +0: compares and keys like +0
}

__device__ __forceinline__ bool mined_keep(float v, int64_t query, int64_t cand, float tau, int64_t cut) {
  return cand == query || v > tau || (v == tau && cand <= cut);
}

// Waves own 32 queries and stream the candidates of one split (softmax_fwd_kernel's loop); MODE selects what is done
// with a tile of logits.  kModeHist runs with ONE wave per workgroup (its LDS histogram), the others with four.
template <int DP, int MODE>
__global__ void __launch_bounds__(256) mined_scan_kernel(const MinedArgs a) {
  const SoftmaxArgs &s = a.s;
  if (MODE == kModeFwd && blockIdx.x == 0 && threadIdx.x == 0) *s.ticket = 0u;  // re-arms the finalize kernel's ticket
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const int64_t nqb = (s.nq + 31) / 32;
  if (wid >= nqb * s.nsplit) return;
  const int64_t qb = wid / s.nsplit;
  const int sp = (int)(wid - qb * s.nsplit);
  const int j = lane & 31, h = lane >> 5;
  const int64_t query = qb * 32 + j;
  const bool qvalid = query < s.nq;
  const bool vec_ok = (s.d == DP) && ((((uintptr_t)s.q) | ((uintptr_t)s.c)) % 16 == 0);

  float tau_r = -__builtin_inff();
  int64_t cut_r = kCutAll;
  if (a.tau && qvalid) {
    tau_r = a.tau[query];
    cut_r = a.cut[query];
  }
  // the cut passes: leave when no row of the wave takes fewer ties than exist / has its r-th tie in this split
  uint32_t want = 0, before = 0;
  bool active = false;
  if constexpr (MODE == kModeTieCount || MODE == kModeTieFind) {
    active = qvalid && a.need[query] != 0u;
    if constexpr (MODE == kModeTieFind) {
      if (active) {
        want = a.krem[query];
        for (int p = 0; p < sp; ++p) before += a.tiecnt[(int64_t)p * s.nq + query];
        const uint32_t mine = a.tiecnt[(int64_t)sp * s.nq + query];
        active = before < want && want <= before + mine;
      }
    }
    if (!__any(active)) return;
  }

  __shared__ uint32_t hist_lds[MODE == kModeHist ? 32 * kHistStride : 1];
  uint32_t prefix_r = 0;
  if constexpr (MODE == kModeHist) {
    for (int i = lane; i < 32 * kHistStride; i += 64) hist_lds[i] = 0u;
    if (qvalid) prefix_r = a.prefix[query];
    __syncthreads();  // one wave per workgroup
  }
  const int shift = 24 - 8 * a.pass;

  float bq[DP / 2];
  load_row_frag<DP>(bq, s.q, query, qvalid, s.d, h, vec_ok);
  const int64_t id_q = (s.ids && qvalid) ? s.ids[query] : 0;

  // kModeCount: the positive logit from the diagonal tile (this wave's queries against candidates qb*32 .. +31), by
  // the arithmetic of every other tile: it ties exactly with copies of itself
  float pos = 0.0f;
  if constexpr (MODE == kModeCount) {
    float ad[DP / 2];
    load_row_frag<DP>(ad, s.c, query, qvalid, s.d, h, vec_ok);  // nq <= nc: a valid query is a valid candidate row
    const f32x16 acc = tile_dot<DP>(ad, bq);
    float own = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (tile_row_of_reg(r, h) == j && qvalid) {
        bool masked;
        own = mined_logit(acc[r], query, query, a, s.corr ? s.corr[query] : 0.0f, id_q, id_q, &masked);
      }
    const float other = __shfl_xor(own, 32);
    pos = (((j >> 2) & 1) == h) ? own : other;  // tile row j lives in lane half (j >> 2) & 1
  }

  float m = -__builtin_inff(), l = 0.0f, fpos = 0.0f;
  bool haspos = false;
  uint32_t count = 0, running = before;
  int64_t found = -1;
  const int64_t c_lo = (int64_t)sp * s.split_len;
  int64_t c_hi = c_lo + s.split_len;
  if (c_hi > s.nc) c_hi = s.nc;

  float af_next[DP / 2];
  load_row_frag<DP>(af_next, s.c, c_lo + j, c_lo + j < s.nc && c_lo < c_hi, s.d, h, vec_ok);
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int k = 0; k < DP / 2; ++k) af[k] = af_next[k];
    if (c0 + 32 < c_hi) load_row_frag<DP>(af_next, s.c, c0 + 32 + j, c0 + 32 + j < s.nc, s.d, h, vec_ok);
    const f32x16 acc = tile_dot<DP>(af, bq);

    float sv[16];
    float tmax = -__builtin_inff();
    uint32_t tiebits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int trow = tile_row_of_reg(r, h);
      const int64_t cand = c0 + trow;
      float kept = -__builtin_inff();
      if (qvalid && cand < c_hi) {
        bool masked;
        const float v = mined_logit(acc[r], query, cand, a, s.corr ? s.corr[cand] : 0.0f, id_q,
                                    s.ids ? s.ids[cand] : 0, &masked);
        if constexpr (MODE == kModeHist) {
          const uint32_t key = f32_orderable(v);
          if (cand != query && (((key ^ prefix_r) >> shift) >> 8) == 0u)
            atomicAdd(&hist_lds[j * kHistStride + ((key >> shift) & 255u)], 1u);
        } else if constexpr (MODE == kModeTieCount || MODE == kModeTieFind) {
          if (cand != query && v == tau_r) tiebits |= 1u << trow;
        } else if constexpr (MODE == kModeCount) {
          if (cand != query && mined_keep(v, query, cand, tau_r, cut_r) && v > pos) ++count;
        } else {
          if (mined_keep(v, query, cand, tau_r, cut_r)) kept = v;
          if (cand == query) {
            fpos = v;
            haspos = true;
          }
        }
      }
      sv[r] = kept;
      tmax = fmaxf(tmax, kept);
    }
    if constexpr (MODE == kModeFwd) {
      if (tmax > m) {
        l *= __expf(m - tmax);
        m = tmax;
      }
      if (m > -__builtin_inff()) {
#pragma unroll
        for (int r = 0; r < 16; ++r) l += __expf(sv[r] - m);
      }
    }
    if constexpr (MODE == kModeTieCount || MODE == kModeTieFind) {
      // a query's 32 candidates of the tile sit in its two lane halves: bit t of `full` = tile row t ties with tau
      const uint32_t full = tiebits | (uint32_t)__shfl_xor((int)tiebits, 32);
      const uint32_t pc = (uint32_t)__popc(full);
      if constexpr (MODE == kModeTieFind) {
        if (active && found < 0 && running + pc >= want) {
          uint32_t bits = full;
          for (uint32_t skip = want - running - 1u; skip > 0u; --skip) bits &= bits - 1u;
          found = c0 + (__ffs((int)bits) - 1);
        }
      }
      running += pc;
    }
  }

  if constexpr (MODE == kModeHist) {
    __syncthreads();
    for (int i = lane; i < 32 * 256; i += 64) {
      const int row = i >> 8, bin = i & 255;
      const uint32_t v = hist_lds[row * kHistStride + bin];
      if (v != 0u && qb * 32 + row < s.nq) atomicAdd(&a.hist[(qb * 32 + row) * 256 + bin], v);
    }
  } else if constexpr (MODE == kModeTieCount) {
    if (h == 0 && qvalid) a.tiecnt[(int64_t)sp * s.nq + query] = running;
  } else if constexpr (MODE == kModeTieFind) {
    if (h == 0 && active && found >= 0) a.cut_w[query] = found;
  } else if constexpr (MODE == kModeCount) {
    const uint32_t total = count + (uint32_t)__shfl_xor((int)count, 32);
    if (h == 0 && qvalid) {
      a.cnt_part[(int64_t)sp * s.nq + query] = total;
      if (sp == 0) s.ppos[query] = pos;
    }
  } else {
    const float m2 = __shfl_xor(m, 32), l2 = __shfl_xor(l, 32);
    const float mm = fmaxf(m, m2);
    float ll = 0.0f;
    if (m > -__builtin_inff()) ll += l * __expf(m - mm);
    if (m2 > -__builtin_inff()) ll += l2 * __expf(m2 - mm);
    if (h == 0 && qvalid) {
      s.pm[(int64_t)sp * s.nq + query] = mm;
      s.pl[(int64_t)sp * s.nq + query] = ll;
    }
    if (haspos) s.ppos[query] = fpos;
  }
}

// Arms the selection: zero bins, empty prefix, wanted rank n.  n = 0 keeps the positive alone: tau = +inf, cut = -1
// are written here and nothing else runs.
__global__ void __launch_bounds__(256) mined_init_kernel(const MinedArgs a, uint32_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n == 0u) {
    for (int64_t row = t0; row < a.s.nq; row += stride) {
      a.tau_w[row] = __builtin_inff();
      a.cut_w[row] = -1;
    }
    return;
  }
  for (int64_t i = t0; i < a.s.nq * 256; i += stride) a.hist[i] = 0u;
  for (int64_t row = t0; row < a.s.nq; row += stride) {
    a.prefix[row] = 0u;
    a.krem[row] = n;
  }
}

// One thread per row: the digit of this pass is the highest bin at which the wanted rank is reached; the bins are
// zeroed for the next pass (and the next call).  After the last pass: tau, whether a cut is needed, cut = all ties.
__global__ void __launch_bounds__(256) mined_pick_kernel(const MinedArgs a) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.s.nq) return;
  uint32_t *bins = a.hist + row * 256;
  uint32_t k = a.krem[row], cnt = 0u;
  int digit = 0;
  bool found = false;
  for (int b = 255; b >= 0; --b) {
    const uint32_t c = bins[b];
    bins[b] = 0u;
    if (!found) {
      if (k <= c) {
        digit = b;
        cnt = c;
        found = true;
      } else {
        k -= c;
      }
    }
  }
  const uint32_t prefix = a.prefix[row] | ((uint32_t)digit << (24 - 8 * a.pass));
  a.prefix[row] = prefix;
  a.krem[row] = k;
  if (a.pass == 3) {
    a.tau_w[row] = f32_from_orderable(prefix);
    a.need[row] = k < cnt ? 1u : 0u;
    a.cut_w[row] = kCutAll;
  }
}

// counts[b] = sum over splits of the partial counts, bit 31 for a non-finite positive (tfrs_rank_count_accumulate's
// convention, consumed by tfrs_topk_hits_update)
__global__ void __launch_bounds__(256) mined_count_reduce_kernel(const MinedArgs a, uint32_t *counts) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.s.nq) return;
  uint32_t total = 0u;
  for (int sp = 0; sp < a.s.nsplit; ++sp) total += a.cnt_part[(int64_t)sp * a.s.nq + row];
  counts[row] = (total & 0x7FFFFFFFu) | (nonfinite_bits(a.s.ppos[row]) << 31);
}

// softmax_bwd_kernel of the 2-D route with keep() applied to every recomputed logit.
// ROWS_ARE_QUERIES = true : wave owns 32 queries, streams candidates, partial dq.
// ROWS_ARE_QUERIES = false: wave owns 32 candidates, streams queries, partial dc.
template <int DP, bool ROWS_ARE_QUERIES>
__global__ void __launch_bounds__(256) mined_bwd_kernel(const MinedArgs a) {
  const SoftmaxArgs &s = a.s;
  constexpr int NFB = (DP + 31) / 32;  // 32-feature output blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nrb = ROWS_ARE_QUERIES ? (s.nq + 31) / 32 : (s.nc + 31) / 32;
  const int64_t n_s = ROWS_ARE_QUERIES ? s.nc : s.nq;
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  if (wid >= nrb * s.nsplit) return;
  const int64_t rb = wid / s.nsplit;
  const int sp = (int)(wid - rb * s.nsplit);
  const int j = lane & 31, h = lane >> 5;
  const bool vec_ok = (s.d == DP) && ((((uintptr_t)s.q) | ((uintptr_t)s.c)) % 16 == 0);

  const int64_t rrow = rb * 32 + j;  // the owned row of q / of c, and of the output
  const bool rvalid = ROWS_ARE_QUERIES ? rrow < s.nq : rrow < s.nc;

  float br[DP / 2];
  load_row_frag<DP>(br, ROWS_ARE_QUERIES ? s.q : s.c, rrow, rvalid, s.d, h, vec_ok);

  // per-lane constants of the owned row
  float lse_r = 0.0f, w_r = 1.0f, corr_r = 0.0f, tau_r = -__builtin_inff();
  int64_t id_r = 0, cut_r = kCutAll;
  if (rvalid) {
    if (ROWS_ARE_QUERIES) {
      lse_r = s.lse[rrow];
      if (s.w) w_r = s.w[rrow];
      if (s.ids) id_r = s.ids[rrow];  // nq <= nc, so a query is also a valid candidate row
      if (a.tau) {
        tau_r = a.tau[rrow];
        cut_r = a.cut[rrow];
      }
    } else {
      if (s.corr) corr_r = s.corr[rrow];
      if (s.ids) id_r = s.ids[rrow];
    }
  }
  const float gl = (s.gloss ? *s.gloss : 1.0f) * s.inv_t;

  f32x16 outacc[NFB];
#pragma unroll
  for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
    for (int r = 0; r < 16; ++r) outacc[fb][r] = 0.0f;

  const int64_t s_lo = (int64_t)sp * s.split_len;
  int64_t s_hi = s_lo + s.split_len;
  if (s_hi > n_s) s_hi = n_s;
  const float *sdata = ROWS_ARE_QUERIES ? s.c : s.q;

  // the streamed tile: one tile ahead in registers (the first GEMM's A fragment), mirrored into this wave's LDS
  // slab so that the second GEMM reads it transposed (lane = feature)
  constexpr int kLd = DP + 4;  // floats per LDS row (+16 B: rows start in different bank groups)
  extern __shared__ __attribute__((aligned(16))) float smem_mined[];
  float *slab = smem_mined + (size_t)wave * 32 * kLd;
  float af_next[DP / 2];
  load_row_frag<DP>(af_next, sdata, s_lo + j, s_lo + j < n_s && s_lo < s_hi, s.d, h, vec_ok);

  for (int64_t s0 = s_lo; s0 < s_hi; s0 += 32) {
    float af[DP / 2];
#pragma unroll
    for (int k = 0; k < DP / 2; ++k) af[k] = af_next[k];
    if (s0 + 32 < s_hi) load_row_frag<DP>(af_next, sdata, s0 + 32 + j, s0 + 32 + j < n_s, s.d, h, vec_ok);
#pragma unroll
    for (int m4 = 0; m4 < DP / 8; ++m4)
      *reinterpret_cast<float4 *>(slab + j * kLd + h * (DP / 2) + 4 * m4) =
          make_float4(af[4 * m4], af[4 * m4 + 1], af[4 * m4 + 2], af[4 * m4 + 3]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x16 acc = tile_dot<DP>(af, br);

    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float gg = 0.0f;
      const int64_t srow = s0 + tile_row_of_reg(r, h);
      if (rvalid && srow < s_hi) {
        const int64_t query = ROWS_ARE_QUERIES ? rrow : srow;
        const int64_t cand = ROWS_ARE_QUERIES ? srow : rrow;
        const float corr_c = ROWS_ARE_QUERIES ? (s.corr ? s.corr[cand] : 0.0f) : corr_r;
        const int64_t id_q = ROWS_ARE_QUERIES ? id_r : (s.ids ? s.ids[query] : 0);
        const int64_t id_c = ROWS_ARE_QUERIES ? (s.ids ? s.ids[cand] : 0) : id_r;
        bool masked;
        const float v = mined_logit(acc[r], query, cand, a, corr_c, id_q, id_c, &masked);
        const float tau_q = ROWS_ARE_QUERIES ? tau_r : (a.tau ? a.tau[query] : -__builtin_inff());
        const int64_t cut_q = ROWS_ARE_QUERIES ? cut_r : (a.tau ? a.cut[query] : kCutAll);
        if (!masked && mined_keep(v, query, cand, tau_q, cut_q)) {
          const float lse_q = ROWS_ARE_QUERIES ? lse_r : s.lse[query];
          const float w_q = ROWS_ARE_QUERIES ? w_r : (s.w ? s.w[query] : 1.0f);
          gg = w_q * (__expf(v - lse_q) - (cand == query ? 1.0f : 0.0f)) * gl;
        }
      }
      g[r] = gg;
    }

    // out^T[feature][owned row] += sum over the 32 streamed rows of X[srow][feature] * G[srow][row]: MFMA step r
    // contracts the streamed-row pair (tile_row_of_reg(r, 0), tile_row_of_reg(r, 1)), where g[r] lives
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
    const int64_t n_out = ROWS_ARE_QUERIES ? s.nq : s.nc;
    float *dst = s.partial + ((int64_t)sp * n_out + rrow) * s.d;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int feat = fb * 32 + tile_row_of_reg(r, h);
        if (feat < s.d) dst[feat] = outacc[fb][r];
      }
  }
}

template <int DP, int MODE>
static void launch_scan(const MinedArgs &a, hipStream_t st) {
  const int64_t waves = ((a.s.nq + 31) / 32) * a.s.nsplit;
  if (MODE == kModeHist)
    hipLaunchKernelGGL((mined_scan_kernel<DP, MODE>), dim3((unsigned)waves), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((mined_scan_kernel<DP, MODE>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a);
}

template <int MODE>
static void scan(const MinedArgs &a, hipStream_t st) {
  for_padded_dim(a.s.d, [&](auto dp) { launch_scan<decltype(dp)::value, MODE>(a, st); });
}

template <int DP, bool RQ>
static void launch_mined_bwd(const MinedArgs &a, hipStream_t st) {
  const int64_t waves = ((RQ ? a.s.nq : a.s.nc) + 31) / 32 * a.s.nsplit;
  const size_t lds = (size_t)4 * 32 * (DP + 4) * sizeof(float);
  hipLaunchKernelGGL((mined_bwd_kernel<DP, RQ>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, st, a);
}

// One workspace serves the four calls (each uses it from the start): the selection's bins and per-row state,
// the forward's partials, the backward's two partial-gradient buffers, the count's partials.
struct MinedLayout {
  int nsq, nsc;
  int64_t lenq, lenc;
  size_t select, fwd, bwd, count;
  size_t bytes() const { return std::max(std::max(select, fwd), std::max(bwd, count)); }
};

static MinedLayout mined_layout(int64_t nq, int64_t nc, int d) {
  MinedLayout L;
  const int64_t target = resolve_target_waves();
  plan_queries(target, nq, 0, nc, &L.nsq, &L.lenq);
  plan_candidates(target, nq, 0, nc, &L.nsc, &L.lenc);
  L.select = al((size_t)nq * 256 * 4) + 3 * al((size_t)nq * 4) + al((size_t)L.nsq * nq * 4);
  L.fwd = 2 * al((size_t)L.nsq * nq * 4) + al((size_t)nq * 4) + al((size_t)((nq + 255) / 256) * 8) + al(4);
  L.bwd = al((size_t)L.nsq * nq * d * 4) + al((size_t)L.nsc * nc * d * 4);
  L.count = al((size_t)L.nsq * nq * 4) + al((size_t)nq * 4);
  return L;
}

static MinedArgs mined_args(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w, float t,
                            const float *corr, const int64_t *ids, const uint8_t *mask, const float *tau,
                            const int64_t *cut) {
  MinedArgs a = {};
  a.s.q = q; a.s.c = c; a.s.nq = nq; a.s.nc = nc; a.s.d = d;
  a.s.w = w; a.s.inv_t = 1.0f / t; a.s.corr = corr; a.s.ids = ids; a.s.mask = mask;
  a.s.heads = 1; a.s.lhp = 0;
  a.t = t; a.tau = tau; a.cut = cut;
  return a;
}

}  // namespace tfrs

using namespace tfrs;

static int mined_check(const float *q, const float *c, int64_t nq, int64_t nc, int d, float t, const void *tau,
                       const void *cut, const void *ws, size_t ws_bytes, const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1 && d >= 1, "%s: bad shape (nq=%lld, nc=%lld, d=%d)", who, (long long)nq,
                 (long long)nc, d);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(d <= TFRS_MAX_DIM, "%s: embedding dim=%d above %d", who, d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  TFRS_CHECK_ARG(t == t && t != 0.0f && t - t == 0.0f, "%s: temperature must be finite and non-zero", who);
  TFRS_CHECK_ARG((tau == nullptr) == (cut == nullptr), "%s: tau and cut come together (both NULL: keep everything)",
                 who);
  TFRS_CHECK_ARG(ws, "%s: NULL workspace", who);
  TFRS_CHECK_ARG(ws_bytes >= mined_layout(nq, nc, d).bytes(), "%s: workspace too small", who);
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_mined_workspace_bytes(int64_t nq, int64_t nc, int d) {
  if (nq < 1 || nc < nq || d < 1 || d > TFRS_MAX_DIM) return 256;
  return mined_layout(nq, nc, d).bytes();
}

extern "C" int tfrs_inbatch_mined_plan(int64_t nq, int64_t nc, int64_t *out) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= nq && out, "inbatch_mined_plan: bad argument");
  const MinedLayout L = mined_layout(nq, nc, 1);
  out[0] = L.nsq; out[1] = L.lenq; out[2] = L.nsc; out[3] = L.lenc;
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_select(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         float temperature, const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, int64_t num_hard_negatives, float *tau,
                                         int64_t *cut, void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_select";
  TFRS_CHECK_ARG(num_hard_negatives >= 0, "%s: num_hard_negatives=%lld is negative", who,
                 (long long)num_hard_negatives);
  TFRS_CHECK_ARG(tau && cut, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, nullptr, temperature, log_q_correction, cand_ids, score_mask, nullptr,
                           nullptr);
  const MinedLayout L = mined_layout(nq, nc, d);
  a.s.nsplit = L.nsq; a.s.split_len = L.lenq;
  char *p = static_cast<char *>(workspace);
  a.hist = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 256 * 4);
  a.prefix = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.krem = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.need = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.tiecnt = reinterpret_cast<uint32_t *>(p);
  a.tau_w = tau; a.cut_w = cut;
  const int64_t n = std::min<int64_t>(num_hard_negatives, nc - 1);  // loss.py:91
  const unsigned row_blocks = (unsigned)((nq + 255) / 256);
  hipLaunchKernelGGL(mined_init_kernel, dim3((unsigned)std::min<int64_t>(nq, 2048)), dim3(256), 0, st, a, (uint32_t)n);
  TFRS_LAUNCH_CHECK();
  if (n == 0) return TFRS_OK;
  for (a.pass = 0; a.pass < 4; ++a.pass) {
    scan<kModeHist>(a, st);
    TFRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mined_pick_kernel, dim3(row_blocks), dim3(256), 0, st, a);
    TFRS_LAUNCH_CHECK();
  }
  a.pass = 0;
  a.tau = tau;  // the cut passes compare with the threshold just written
  a.cut = cut;
  scan<kModeTieCount>(a, st);
  TFRS_LAUNCH_CHECK();
  scan<kModeTieFind>(a, st);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         const float *sample_weight, float temperature,
                                         const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, const float *tau, const int64_t *cut,
                                         float *out_loss, float *out_lse, float *out_pos, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_ce_fwd";
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, sample_weight, temperature, log_q_correction, cand_ids, score_mask, tau,
                           cut);
  const MinedLayout L = mined_layout(nq, nc, d);
  a.s.nsplit = L.nsq; a.s.split_len = L.lenq;
  char *p = static_cast<char *>(workspace);
  a.s.pm = reinterpret_cast<float *>(p); p += al((size_t)L.nsq * nq * 4);
  a.s.pl = reinterpret_cast<float *>(p); p += al((size_t)L.nsq * nq * 4);
  a.s.ppos = reinterpret_cast<float *>(p); p += al((size_t)nq * 4);
  double *block_part = reinterpret_cast<double *>(p); p += al((size_t)((nq + 255) / 256) * 8);
  a.s.ticket = reinterpret_cast<uint32_t *>(p);
  scan<kModeFwd>(a, st);
  TFRS_LAUNCH_CHECK();
  softmax_launch_finalize(a.s, out_loss, out_lse, out_pos, block_part, st);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         const float *sample_weight, float temperature,
                                         const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, const float *tau, const int64_t *cut,
                                         const float *lse, const float *gloss, float *dq, float *dc, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_ce_bwd";
  TFRS_CHECK_ARG(lse && dq && dc, "%s: NULL pointer", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, sample_weight, temperature, log_q_correction, cand_ids, score_mask, tau,
                           cut);
  a.s.lse = lse; a.s.gloss = gloss;
  const MinedLayout L = mined_layout(nq, nc, d);
  char *p = static_cast<char *>(workspace);
  // dq: waves own query blocks, stream candidates
  a.s.nsplit = L.nsq; a.s.split_len = L.lenq;
  a.s.partial = reinterpret_cast<float *>(p);
  for_padded_dim(d, [&](auto dp) { launch_mined_bwd<decltype(dp)::value, true>(a, st); });
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.s.partial, a.s.nsplit, nq * d, dq, st);
  TFRS_LAUNCH_CHECK();
  // dc: waves own candidates, stream queries
  p += al((size_t)L.nsq * nq * d * 4);
  a.s.nsplit = L.nsc; a.s.split_len = L.lenc;
  a.s.partial = reinterpret_cast<float *>(p);
  for_padded_dim(d, [&](auto dp) { launch_mined_bwd<decltype(dp)::value, false>(a, st); });
  TFRS_LAUNCH_CHECK();
  softmax_launch_reduce(a.s.partial, a.s.nsplit, nc * d, dc, st);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_rank_count(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                             float temperature, const float *log_q_correction,
                                             const int64_t *cand_ids, const uint8_t *score_mask, const float *tau,
                                             const int64_t *cut, uint32_t *counts, void *workspace,
                                             size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_rank_count";
  TFRS_CHECK_ARG(counts, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, nullptr, temperature, log_q_correction, cand_ids, score_mask, tau, cut);
  const MinedLayout L = mined_layout(nq, nc, d);
  a.s.nsplit = L.nsq; a.s.split_len = L.lenq;
  char *p = static_cast<char *>(workspace);
  a.cnt_part = reinterpret_cast<uint32_t *>(p); p += al((size_t)L.nsq * nq * 4);
  a.s.ppos = reinterpret_cast<float *>(p);
  scan<kModeCount>(a, st);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mined_count_reduce_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, a, counts);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
