// attention.hip -- the core of a Keras MultiHeadAttention layer, softmax(scale Q K^T + masks) V per (batch row, head),
// and its backward, each as ONE launch (layers/attention.py).  Not the max-sim "multi-head" queries of
// tasks.Retrieval / BruteForce: those have no softmax over keys and live in softmax.hip / topk_*.hip.
//
//   q [B, Tq, H, dk]   k [B, Tk, H, dk]   v [B, Tk, H, dv]   out [B, Tq, H, dv]   lse [B, H, Tq]
//
// are the [B T, H d] outputs of the projection GEMMs as they are: a kernel reads its head's strided slice.
// Tq, Tk <= 128 and dk, dv <= 64: everything one (b, h) needs fits in LDS and registers, the scores never leave
// registers.  Products run on v_mfma_f32_32x32x2_f32 (A: lane = row i, lane half = k; B: lane = column j, lane half = k;
// D: lane = column j, register r = row tile_row_of_reg(r, half)).
//
// Forward: a wave owns 32 query rows against all keys.  It computes the strip TRANSPOSED, S^T = K Q^T (A = key rows
// from LDS, B = the wave's query fragment in registers), so a lane holds ONE query and its registers that query's keys
// (the two lane halves hold disjoint keys): row max and row sum are register reductions plus one exchange between the
// halves, and the probabilities already ARE the A operand of P V when the k order of that product is permuted to
// "step (tile, r) takes key tile_row_of_reg(r, half) from lane half `half`", with the V rows read from LDS in the same
// order.  The waves of one (b, h) share one LDS image of K and V; when Tq <= 32 the waves of a workgroup take
// different (b, h) pairs, each with its own image.
//
// Backward: one workgroup per (b, h) with LDS images of Q, dO, K, V and the rows' lse and delta = rowsum(dO o O).
// Waves [0, nq) own query strips (lane = query): per key tile they recompute S^T and P^T = exp(S^T - lse), form
// dP^T = V dO^T, dS = P o (dP - delta) and accumulate dQ = scale dS K with the dS registers as the A operand.
// Waves [nq, nq + nk) own key strips (lane = key): per query tile S = Q K^T, P, dP = dO V^T, dS, and dV = P^T dO,
// dK = scale dS^T Q, again from registers.  P comes from the saved lse, so no role needs a row reduction and a tile of
// 16 registers is all of S that is live.  The scores are computed twice (seven products where five would do): the
// price of having no reduction across waves.  No atomics, no workspace: every output element has exactly one writer.
//
// A query row with no allowed key gives out = +0, lse = +inf and zero gradients (Keras gives the mean of V).
#include <cmath>

#include "common.h"
#include "mfma_tile.h"

namespace tfrs {

struct AttnArgs {
  const float *q, *k, *v;
  const uint8_t *am, *qm, *km;      // [B, Tq, Tk], [B, Tq], [B, Tk]; 1 = attend; each may be NULL
  int64_t pairs;                    // B * H
  int Tq, Tk, H, dk, dv, causal;
  float scale;
  float *out, *lse;                 // forward: written.  backward: read
  const float *dout;                // backward only from here on
  float *dq, *dkey, *dv_out;
};

struct Bits128 {
  uint64_t lo, hi;
  __device__ __forceinline__ bool test(int i) const { return ((i < 64 ? lo >> i : hi >> (i - 64)) & 1ull) != 0; }
};

// bit i: i < n and m[i] != 0 (no mask: i < n).  The whole wave calls it; the result is the same in every lane.
__device__ __forceinline__ Bits128 attn_row_bits(const uint8_t *m, int n, int lane) {
  Bits128 b;
  b.lo = __ballot(lane < n && (!m || m[lane] != 0));
  b.hi = __ballot(lane + 64 < n && (!m || m[lane + 64] != 0));
  return b;
}

// rows [0, rows) of a head's strided slice into a zero-padded LDS image of pitch DP + 1
template <int DP>
__device__ __forceinline__ void attn_stage(float *img, int rows, const float *src, int live, int64_t ld, int d, int tid,
                                           int nthreads) {
  for (int idx = tid; idx < rows * DP; idx += nthreads) {
    const int row = idx / DP, f = idx % DP;
    img[row * (DP + 1) + f] = (row < live && f < d) ? src[row * ld + f] : 0.0f;
  }
}

// element [row][col] of an image as the B operand of an output tile 32 wide: columns past DP (DP = 16) are zero
template <int DP>
__device__ __forceinline__ float attn_col(const float *img, int row, int col) {
  return (DP >= 32 || col < DP) ? img[row * (DP + 1) + col] : 0.0f;
}

template <int NT, int DP>
__global__ void __launch_bounds__(256) attention_fwd_kernel(AttnArgs a, int pack) {
  constexpr int KH = DP / 2, P = DP + 1, ROWS = NT * 32, NV = DP >= 64 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int Tq = a.Tq, Tk = a.Tk, H = a.H, dk = a.dk, dv = a.dv;
  // pack > 0: Tq <= 32 and wave w of the workgroup has pair blockIdx.x * pack + w and an image of its own
  const int64_t pair = pack ? (int64_t)blockIdx.x * pack + wave : (int64_t)blockIdx.x;
  const int strip = pack ? 0 : wave;
  const bool has_pair = pair < a.pairs;
  const int64_t b = has_pair ? pair / H : 0;
  const int h = has_pair ? (int)(pair % H) : 0;
  float *Ks = attn_lds + (pack ? wave * (2 * ROWS * P) : 0), *Vs = Ks + ROWS * P;
  if (has_pair) {
    const int tid = pack ? lane : (int)threadIdx.x, nthreads = pack ? 64 : (int)blockDim.x;
    attn_stage<DP>(Ks, ROWS, a.k + (b * Tk * H + h) * dk, Tk, (int64_t)H * dk, dk, tid, nthreads);
    attn_stage<DP>(Vs, ROWS, a.v + (b * Tk * H + h) * dv, Tk, (int64_t)H * dv, dv, tid, nthreads);
  }
  __syncthreads();
  if (!has_pair || strip * 32 >= Tq) return;

  const int query = strip * 32 + jl;
  const bool qok = query < Tq;
  float qf[KH];
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    const int f = hh * KH + s;
    qf[s] = (qok && f < dk) ? a.q[((b * Tq + query) * H + h) * dk + f] : 0.0f;
  }
  f32x16 sc[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[kt][r] = 0.0f;
    const float *krow = &Ks[(kt * 32 + jl) * P + hh * KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[s], qf[s], sc[kt], 0, 0, 0);
  }

  const Bits128 kbits = attn_row_bits(a.km ? a.km + b * Tk : nullptr, Tk, lane);
  const bool qallow = qok && (!a.qm || a.qm[b * Tq + query] != 0);
  const uint8_t *amrow = a.am ? a.am + (b * Tq + (qok ? query : 0)) * Tk : nullptr;
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + tile_row_of_reg(r, hh);
      const bool ok = qallow && kbits.test(key) && (!a.causal || key <= query) && (!amrow || amrow[key] != 0);
      sc[kt][r] = ok ? __fmul_rn(a.scale, sc[kt][r]) : -INFINITY;
      m = fmaxf(m, sc[kt][r]);
    }
  m = fmaxf(m, __shfl_xor(m, 32));
  const float base = m == -INFINITY ? 0.0f : m;       // a row with nothing allowed: every exp below is exp(-inf) = +0
  float l = 0.0f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sc[kt][r] = expf(__fsub_rn(sc[kt][r], base));
      l += sc[kt][r];
    }
  l += __shfl_xor(l, 32);
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  if (hh == 0 && qok) a.lse[pair * Tq + query] = l > 0.0f ? base + logf(l) : INFINITY;

  // out = P V: step (kt, r) takes P[query][key] from the lane that holds it and V[key][column] from LDS
  f32x16 o[NV];
#pragma unroll
  for (int nv = 0; nv < NV; ++nv)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nv][r] = 0.0f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + tile_row_of_reg(r, hh);
      const float p = sc[kt][r] * inv;
#pragma unroll
      for (int nv = 0; nv < NV; ++nv)
        o[nv] = __builtin_amdgcn_mfma_f32_32x32x2f32(p, attn_col<DP>(Vs, key, nv * 32 + jl), o[nv], 0, 0, 0);
    }
#pragma unroll
  for (int nv = 0; nv < NV; ++nv)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = strip * 32 + tile_row_of_reg(r, hh), n = nv * 32 + jl;
      if (row < Tq && n < dv) a.out[((b * Tq + row) * H + h) * dv + n] = o[nv][r];
    }
}

template <int DP>
__global__ void __launch_bounds__(512) attention_bwd_kernel(AttnArgs a) {
  constexpr int KH = DP / 2, P = DP + 1, NV = DP >= 64 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int Tq = a.Tq, Tk = a.Tk, H = a.H, dk = a.dk, dv = a.dv;
  const int nq = (Tq + 31) / 32, nk = (Tk + 31) / 32, RQ = nq * 32, RK = nk * 32;
  float *Qs = attn_lds, *dOs = Qs + RQ * P, *Ks = dOs + RQ * P, *Vs = Ks + RK * P;
  float *lse_s = Vs + RK * P, *delta_s = lse_s + RQ;
  const int64_t pair = blockIdx.x, b = pair / H;
  const int h = (int)(pair % H);
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int64_t qbase = (b * Tq * H + h), kbase = (b * Tk * H + h);
  attn_stage<DP>(Qs, RQ, a.q + qbase * dk, Tq, (int64_t)H * dk, dk, tid, nthreads);
  attn_stage<DP>(dOs, RQ, a.dout + qbase * dv, Tq, (int64_t)H * dv, dv, tid, nthreads);
  attn_stage<DP>(Ks, RK, a.k + kbase * dk, Tk, (int64_t)H * dk, dk, tid, nthreads);
  attn_stage<DP>(Vs, RK, a.v + kbase * dv, Tk, (int64_t)H * dv, dv, tid, nthreads);
  for (int i = tid; i < RQ; i += nthreads) lse_s[i] = i < Tq ? a.lse[pair * Tq + i] : INFINITY;
  // delta = rowsum(dO o O) is the diagonal of the tile dO O^T, taken on the matrix cores in the k order of dP: a row
  // with ONE allowed key has P = 1 and O = V bit for bit, so its dP - delta, dS and gradients are zero exactly
  float gf[KH];
  if (wave < nq) {
    const int query = wave * 32 + jl;
    float of[KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      const int f = hh * KH + s;
      const bool ok = query < Tq && f < dv;
      of[s] = ok ? a.out[(qbase + (int64_t)query * H) * dv + f] : 0.0f;
      gf[s] = ok ? a.dout[(qbase + (int64_t)query * H) * dv + f] : 0.0f;
    }
    const f32x16 dl = tile_dot<DP>(of, gf);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (tile_row_of_reg(r, hh) == jl) delta_s[query] = dl[r];
  }
  __syncthreads();

  f32x16 acc0[NV], acc1[NV];
#pragma unroll
  for (int nv = 0; nv < NV; ++nv)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[nv][r] = acc1[nv][r] = 0.0f;

  if (wave < nq) {
    // ---- query-owned strip: lane = query, registers = keys of the current key tile; acc0 = dQ ----
    const int q0 = wave * 32, query = q0 + jl;
    const bool qok = query < Tq;
    const bool qallow = qok && (!a.qm || a.qm[b * Tq + query] != 0);
    const uint8_t *amrow = a.am ? a.am + (b * Tq + (qok ? query : 0)) * Tk : nullptr;
    const Bits128 kbits = attn_row_bits(a.km ? a.km + b * Tk : nullptr, Tk, lane);
    const float lse = lse_s[query], delta = delta_s[query];
    float qf[KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) qf[s] = Qs[query * P + hh * KH + s];
    for (int kt = 0; kt < nk; ++kt) {
      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.0f;
      const float *krow = &Ks[(kt * 32 + jl) * P + hh * KH], *vrow = &Vs[(kt * 32 + jl) * P + hh * KH];
#pragma unroll
      for (int s = 0; s < KH; ++s) {
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[s], qf[s], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[s], gf[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + tile_row_of_reg(r, hh);
        const bool ok = qallow && kbits.test(key) && (!a.causal || key <= query) && (!amrow || amrow[key] != 0);
        const float p = ok ? expf(__fsub_rn(__fmul_rn(a.scale, st[r]), lse)) : 0.0f;
        const float ds = ok ? a.scale * (p * (dp[r] - delta)) : 0.0f;
#pragma unroll
        for (int nv = 0; nv < NV; ++nv)
          acc0[nv] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds, attn_col<DP>(Ks, key, nv * 32 + jl), acc0[nv], 0, 0, 0);
      }
    }
#pragma unroll
    for (int nv = 0; nv < NV; ++nv)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = q0 + tile_row_of_reg(r, hh), n = nv * 32 + jl;
        if (row < Tq && n < dk) a.dq[(qbase + (int64_t)row * H) * dk + n] = acc0[nv][r];
      }
  } else if (wave < nq + nk) {
    // ---- key-owned strip: lane = key, registers = queries of the current query tile; acc0 = dV, acc1 = dK ----
    const int k0 = (wave - nq) * 32, key = k0 + jl;
    const bool kallow = key < Tk && (!a.km || a.km[b * Tk + key] != 0);
    const Bits128 qbits = attn_row_bits(a.qm ? a.qm + b * Tq : nullptr, Tq, lane);
    const uint8_t *amcol = a.am ? a.am + b * Tq * Tk + (key < Tk ? key : 0) : nullptr;
    float kf[KH], vf[KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      kf[s] = Ks[key * P + hh * KH + s];
      vf[s] = Vs[key * P + hh * KH + s];
    }
    for (int qt = 0; qt < nq; ++qt) {
      f32x16 sv, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) sv[r] = dp[r] = 0.0f;
      const float *qrow = &Qs[(qt * 32 + jl) * P + hh * KH], *grow = &dOs[(qt * 32 + jl) * P + hh * KH];
#pragma unroll
      for (int s = 0; s < KH; ++s) {
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[s], kf[s], sv, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[s], vf[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int query = qt * 32 + tile_row_of_reg(r, hh);
        const bool ok = kallow && qbits.test(query) && (!a.causal || key <= query) &&
                        (!amcol || amcol[(int64_t)query * Tk] != 0);
        const float p = ok ? expf(__fsub_rn(__fmul_rn(a.scale, sv[r]), lse_s[query])) : 0.0f;
        const float ds = ok ? a.scale * (p * (dp[r] - delta_s[query])) : 0.0f;
#pragma unroll
        for (int nv = 0; nv < NV; ++nv) {
          acc0[nv] = __builtin_amdgcn_mfma_f32_32x32x2f32(p, attn_col<DP>(dOs, query, nv * 32 + jl), acc0[nv], 0, 0, 0);
          acc1[nv] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds, attn_col<DP>(Qs, query, nv * 32 + jl), acc1[nv], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int nv = 0; nv < NV; ++nv)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = k0 + tile_row_of_reg(r, hh), n = nv * 32 + jl;
        if (row < Tk && n < dv) a.dv_out[(kbase + (int64_t)row * H) * dv + n] = acc0[nv][r];
        if (row < Tk && n < dk) a.dkey[(kbase + (int64_t)row * H) * dk + n] = acc1[nv][r];
      }
  }
}

constexpr int kAttnLdsLimit = 160 * 1024;      // the LDS of a gfx950 compute unit

template <int NT, int DP>
static int attention_launch_fwd(const AttnArgs &a, hipStream_t stream) {
  constexpr int region = 2 * NT * 32 * (DP + 1) * (int)sizeof(float);
  // Tq <= 32: as many (b, h) pairs per workgroup as there are waves (4), or the 2 that fit at the largest image
  constexpr int max_pack = 4 * region <= kAttnLdsLimit ? 4 : 2;
  const int pack = a.Tq <= 32 ? max_pack : 0;
  const int waves = pack ? pack : (a.Tq + 31) / 32;
  const int lds = (pack ? pack : 1) * region;
  const int64_t blocks = pack ? (a.pairs + pack - 1) / pack : a.pairs;
  TFRS_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(&attention_fwd_kernel<NT, DP>), max_pack * region));
  hipLaunchKernelGGL((attention_fwd_kernel<NT, DP>), dim3((unsigned)blocks), dim3(waves * 64), lds, stream, a, pack);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

template <int DP>
static int attention_dispatch_fwd(const AttnArgs &a, hipStream_t stream) {
  if (a.Tk <= 32) return attention_launch_fwd<1, DP>(a, stream);
  if (a.Tk <= 64) return attention_launch_fwd<2, DP>(a, stream);
  return attention_launch_fwd<4, DP>(a, stream);
}

template <int DP>
static int attention_launch_bwd(const AttnArgs &a, hipStream_t stream) {
  constexpr int max_lds = (4 * TFRS_ATTENTION_MAX_SEQ * (DP + 1) + 2 * TFRS_ATTENTION_MAX_SEQ) * (int)sizeof(float);
  const int nq = (a.Tq + 31) / 32, nk = (a.Tk + 31) / 32;
  const int lds = (2 * (nq + nk) * 32 * (DP + 1) + 2 * nq * 32) * (int)sizeof(float);
  TFRS_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(&attention_bwd_kernel<DP>), max_lds));
  hipLaunchKernelGGL((attention_bwd_kernel<DP>), dim3((unsigned)a.pairs), dim3((nq + nk) * 64), lds, stream, a);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// TFRS_OK with *launch = false: nothing to do.  The envelope comes first: it holds for empty batches too.
static int attention_check_shape(const char *who, int64_t batch, int tq, int tk, int heads, int dk, int dv,
                                 bool *launch) {
  *launch = false;
  TFRS_CHECK_ARG(batch >= 0 && tq >= 0 && tk >= 0 && heads >= 1 && dk >= 1 && dv >= 1, "%s: bad shape", who);
  const struct { const char *name; int value, limit; } limits[] = {
      {"Tq", tq, TFRS_ATTENTION_MAX_SEQ}, {"Tk", tk, TFRS_ATTENTION_MAX_SEQ},
      {"dk", dk, TFRS_ATTENTION_MAX_HEAD_DIM}, {"dv", dv, TFRS_ATTENTION_MAX_HEAD_DIM}};
  for (const auto &l : limits)
    if (l.value > l.limit) {
      set_error("%s: %s = %d is above the %d the attention kernels hold on chip", who, l.name, l.value, l.limit);
      return TFRS_ENOTIMPL;
    }
  if (batch == 0 || tq == 0) return TFRS_OK;
  TFRS_CHECK_ARG(tk >= 1, "%s: Tk = 0 with queries to serve", who);
  TFRS_CHECK_ARG(batch * heads <= (int64_t)0x7FFFFFFF, "%s: batch * heads too large", who);
  *launch = true;
  return TFRS_OK;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_attention_fwd(const float *q, const float *k, const float *v, const uint8_t *attn_mask,
                                  const uint8_t *q_mask, const uint8_t *k_mask, int64_t B, int Tq, int Tk, int H,
                                  int dk, int dv, float scale, int causal, float *out, float *lse, void *stream) {
  bool launch;
  const int rc = attention_check_shape("attention_fwd", B, Tq, Tk, H, dk, dv, &launch);
  if (rc != TFRS_OK || !launch) return rc;
  TFRS_CHECK_ARG(q && k && v && out && lse, "attention_fwd: NULL pointer");
  AttnArgs a{q, k, v, attn_mask, q_mask, k_mask, B * H, Tq, Tk, H, dk, dv, causal ? 1 : 0, scale, out, lse,
             nullptr, nullptr, nullptr, nullptr};
  switch (softmax_padded_dim(dk > dv ? dk : dv)) {
    case 8:
    case 16: return attention_dispatch_fwd<16>(a, (hipStream_t)stream);
    case 32: return attention_dispatch_fwd<32>(a, (hipStream_t)stream);
    default: return attention_dispatch_fwd<64>(a, (hipStream_t)stream);
  }
}

extern "C" int tfrs_attention_bwd(const float *q, const float *k, const float *v, const uint8_t *attn_mask,
                                  const uint8_t *q_mask, const uint8_t *k_mask, const float *out, const float *lse,
                                  const float *dout, int64_t B, int Tq, int Tk, int H, int dk, int dv, float scale,
                                  int causal, float *dq, float *dkey, float *dv_out, void *stream) {
  bool launch;
  const int rc = attention_check_shape("attention_bwd", B, Tq, Tk, H, dk, dv, &launch);
  if (rc != TFRS_OK || !launch) return rc;
  TFRS_CHECK_ARG(q && k && v && out && lse && dout && dq && dkey && dv_out, "attention_bwd: NULL pointer");
  AttnArgs a{q, k, v, attn_mask, q_mask, k_mask, B * H, Tq, Tk, H, dk, dv, causal ? 1 : 0, scale,
             const_cast<float *>(out), const_cast<float *>(lse), dout, dq, dkey, dv_out};
  switch (softmax_padded_dim(dk > dv ? dk : dv)) {
    case 8:
    case 16: return attention_launch_bwd<16>(a, (hipStream_t)stream);
    case 32: return attention_launch_bwd<32>(a, (hipStream_t)stream);
    default: return attention_launch_bwd<64>(a, (hipStream_t)stream);
  }
}
