// lstm.hip -- the recurrence of a Keras LSTM (tanh / sigmoid, gate order i, f, c, o, one bias) and its backward walk,
// each as ONE launch over all T time steps.
//
//   p   = a + h_{t-1} @ R                       R = recurrent_kernel [U, 4U]
//   i   = sigmoid(p_i);  f = sigmoid(p_f);  g = tanh(p_c);  o = sigmoid(p_o)
//   c_t = f * c_{t-1} + i * g;  h_t = o * tanh(c_t)      a = x_t @ kernel + bias: a GEMM the caller ran over all t
//   mask[b, t] == 0:  h_t = h_{t-1}, c_t = c_{t-1}; the sequence output repeats (zeros before the first live step)
//
// Work mapping: a workgroup owns 32 batch rows (the mfma_tile.h tile) and walks the T steps; wave w owns hidden
// columns [32 w, 32 w + 32) of ALL FOUR gates, so the activations, the cell update and the mask select of a column
// are register arithmetic of the lane that holds it (lane = column, 16 accumulator registers = 16 of the 32 rows).
// c lives in those registers only: it never enters a product and never touches LDS.  The products run on
// v_mfma_f32_32x32x2_f32 in the half-split k order of mfma_tile.h: A = the h tile (forward) or the tile of the four
// pre-activation gradients (backward), read from LDS, the only data that crosses waves; B = the wave's slice of R, a
// register fragment read from HBM once per workgroup (4 UP / 2 registers per lane; UP = U padded to 8 / 16 / 32 / 64).
// The pre-activation gradient da is ONE tensor: the input side and the recurrent side of an LSTM share it.
// No atomics, no workspace: every output element is written by exactly one lane.
#include "common.h"
#include "mfma_tile.h"

namespace tfrs {

struct LstmFwdArgs {
  const float *xp;        // [B, T, 4U] input projection, bias included
  const float *rk;        // [U, 4U]
  const uint8_t *mask;    // [B, T] or NULL
  const float *h0, *c0;   // [B, U] or NULL
  int64_t B;
  int T, U, backwards;
  float *seq;             // [B, T, U] in processing order, or NULL
  float *last_h, *last_c; // [B, U]
  float *si, *sf, *sg, *so, *scp, *shp;   // [B, T, U] by time index (training forward), or all NULL
};

struct LstmBwdArgs {
  const float *rk;
  const uint8_t *mask;
  const float *si, *sf, *sg, *so, *scp;
  const float *dseq;      // [B, T, U] in processing order, or NULL
  const float *dlast_h;   // [B, U] or NULL
  const float *dlast_c;   // [B, U] or NULL
  int64_t B;
  int T, U, backwards;
  float *da;              // [B, T, 4U]  (da_i, da_f, da_c, da_o)
  float *dh0, *dc0;       // [B, U]
};

__device__ __forceinline__ float lstm_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

template <int UP> struct LstmCfg {
  static constexpr int kWaves = UP <= 32 ? 1 : UP / 32;
  static constexpr int kBwdLdsBytes = 2 * 32 * (4 * UP + 1) * (int)sizeof(float);
};

// bit i of the result: mask of tile row i at time index tt (all ones without a mask)
__device__ __forceinline__ uint32_t lstm_row_mask(const uint8_t *mask, int64_t row0, int64_t B, int T, int tt,
                                                  int jl) {
  if (!mask) return 0xFFFFFFFFu;
  const int64_t row = row0 + jl;
  const bool m = row < B && mask[row * T + tt] != 0;
  return (uint32_t)__ballot(m);
}

template <int UP, bool TRAIN>
__global__ void __launch_bounds__(LstmCfg<UP>::kWaves * 64) lstm_fwd_kernel(LstmFwdArgs a) {
  constexpr int KH = UP / 2, PITCH = UP + 1;
  __shared__ float hs[2][32 * PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int col = wave * 32 + jl;
  const int U = a.U, T = a.T;
  const bool col_ok = col < U;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int64_t ld = 4 * (int64_t)U;

  // B fragment: R[k = hh * KH + s][g * U + col]; zero for padded k and padded columns
  float w[4][KH];
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    const int k = hh * KH + s;
    const bool ok = col_ok && k < U;
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g][s] = ok ? a.rk[k * ld + g * U + col] : 0.0f;
  }

  float h[16], c[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int tr = tile_row_of_reg(r, hh);
    const int64_t row = row0 + tr;
    const bool ok = col_ok && row < a.B;
    h[r] = (a.h0 && ok) ? a.h0[row * U + col] : 0.0f;
    c[r] = (a.c0 && ok) ? a.c0[row * U + col] : 0.0f;
    if (col < UP) hs[0][tr * PITCH + col] = h[r];
  }

  uint32_t seen = a.mask ? 0u : 0xFFFFFFFFu;     // rows that have had a live step: their output is h, else zero
  for (int t = 0; t < T; ++t) {
    const int tt = a.backwards ? T - 1 - t : t;
    const int cur = t & 1;
    // the step's 64 projection loads go out ahead of the barrier and the products and are first read after them
    float av[4][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + tile_row_of_reg(r, hh);
      const bool ok = col_ok && row < a.B;
#pragma unroll
      for (int g = 0; g < 4; ++g) av[g][r] = ok ? a.xp[(row * T + tt) * ld + g * U + col] : 0.0f;
    }
    const uint32_t live = lstm_row_mask(a.mask, row0, a.B, T, tt, jl);
    seen |= live;
    __syncthreads();     // hs[cur] is complete; every wave has finished reading hs[cur ^ 1]
    f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;
    const float *hrow = &hs[cur][jl * PITCH + hh * KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      const float af = hrow[s];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, w[g][s], acc[g], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = tile_row_of_reg(r, hh);
      const int64_t row = row0 + tr;
      const bool ok = col_ok && row < a.B;
      const float hp = h[r], cp = c[r];
      const float gi = lstm_sigmoid(av[0][r] + acc[0][r]);
      const float gf = lstm_sigmoid(av[1][r] + acc[1][r]);
      const float gg = tanhf(av[2][r] + acc[2][r]);
      const float go = lstm_sigmoid(av[3][r] + acc[3][r]);
      const float cn = __builtin_fmaf(gf, cp, gi * gg);     // spelled out: the backward forms c_t again, bit for bit
      const float hn = go * tanhf(cn);
      const bool on = (live >> tr) & 1u;
      const float hv = on ? hn : hp;
      h[r] = hv;
      c[r] = on ? cn : cp;
      if (ok) {
        if (TRAIN) {
          const int64_t o = (row * T + tt) * U + col;
          a.si[o] = gi;
          a.sf[o] = gf;
          a.sg[o] = gg;
          a.so[o] = go;
          a.scp[o] = cp;
          a.shp[o] = hp;
        }
        if (a.seq) a.seq[(row * T + t) * U + col] = ((seen >> tr) & 1u) ? hv : 0.0f;
      }
      if (col < UP) hs[cur ^ 1][tr * PITCH + col] = col_ok ? hv : 0.0f;
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    if (col_ok && row < a.B) {
      a.last_h[row * U + col] = h[r];
      a.last_c[row * U + col] = c[r];
    }
  }
}

// dh_prev[b][n] = sum_{g, j} da[b][g][j] * R[n][g U + j]: A = the da tile [32, 4 UP] through LDS, B = row n of R
// (contiguous in memory).  dc_prev = dc f.  A masked step stores zeros and passes dh and dc through: its accumulator
// starts at dh and every product of the chain is with a zero.
template <int UP>
__global__ void __launch_bounds__(LstmCfg<UP>::kWaves * 64) lstm_bwd_kernel(LstmBwdArgs a) {
  constexpr int KH = 2 * UP, PITCH = 4 * UP + 1;
  extern __shared__ __attribute__((aligned(16))) float lstm_gs[];      // [2][32 * PITCH]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int col = wave * 32 + jl;
  const int U = a.U, T = a.T;
  const bool col_ok = col < U;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int64_t ld = 4 * (int64_t)U;

  // B fragment: k = hh * KH + s = g * UP + j  ->  R[col][g * U + j]
  float w[KH];
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    const int k = hh * KH + s, g = k / UP, j = k % UP;
    w[s] = (col_ok && j < U) ? a.rk[col * ld + g * U + j] : 0.0f;
  }

  // processing step of the row's first live step: the outputs before it are constant zeros and take no gradient
  int first = 0;
  if (a.mask) {
    first = T;
    const int64_t row = row0 + jl;
    if (row < a.B)
      for (int p = T - 1; p >= 0; --p) {
        const int tp = a.backwards ? T - 1 - p : p;
        first = a.mask[row * T + tp] ? p : first;
      }
  }

  float dh[16], dc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    const bool ok = col_ok && row < a.B;
    dh[r] = (a.dlast_h && ok) ? a.dlast_h[row * U + col] : 0.0f;
    dc[r] = (a.dlast_c && ok) ? a.dlast_c[row * U + col] : 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    const int tt = a.backwards ? T - 1 - t : t;
    float *gbuf = lstm_gs + (t & 1) * (32 * PITCH);     // two buffers, ONE barrier per step, as the forward's h tile
    const uint32_t live = lstm_row_mask(a.mask, row0, a.B, T, tt, jl);
    const uint32_t seen = (uint32_t)__ballot(first <= t);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = tile_row_of_reg(r, hh);
      const int64_t row = row0 + tr;
      const bool ok = col_ok && row < a.B;
      const bool on = ok && ((live >> tr) & 1u);
      float d = dh[r];
      float dai = 0.0f, daf = 0.0f, dag = 0.0f, dao = 0.0f;
      if (ok) {
        if (a.dseq && ((seen >> tr) & 1u)) d += a.dseq[(row * T + t) * U + col];
        if (on) {
          const int64_t o = (row * T + tt) * U + col;
          const float gi = a.si[o], gf = a.sf[o], gg = a.sg[o], go = a.so[o], cp = a.scp[o];
          const float tc = tanhf(__builtin_fmaf(gf, cp, gi * gg));      // tanh(c_t) again, from what the forward saved
          const float dct = dc[r] + d * go * (1.0f - tc * tc);
          dai = dct * gg * gi * (1.0f - gi);
          daf = dct * cp * gf * (1.0f - gf);
          dag = dct * gi * (1.0f - gg * gg);
          dao = d * tc * go * (1.0f - go);
          dc[r] = dct * gf;
        }
        const int64_t o4 = (row * T + tt) * ld + col;
        a.da[o4] = dai;
        a.da[o4 + U] = daf;
        a.da[o4 + 2 * U] = dag;
        a.da[o4 + 3 * U] = dao;
      }
      acc[r] = on ? 0.0f : d;
      if (col < UP) {
        float *grow = &gbuf[tr * PITCH + col];
        grow[0] = dai;
        grow[UP] = daf;
        grow[2 * UP] = dag;
        grow[3 * UP] = dao;
      }
    }
    __syncthreads();
    const float *grow = &gbuf[jl * PITCH + hh * KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[s], w[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = acc[r];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    if (col_ok && row < a.B) {
      a.dh0[row * U + col] = dh[r];
      a.dc0[row * U + col] = dc[r];
    }
  }
}

template <int UP>
static int lstm_launch_fwd(const LstmFwdArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.B + 31) / 32)), block(LstmCfg<UP>::kWaves * 64);
  if (a.si)
    hipLaunchKernelGGL((lstm_fwd_kernel<UP, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((lstm_fwd_kernel<UP, false>), grid, block, 0, stream, a);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

template <int UP>
static int lstm_launch_bwd(const LstmBwdArgs &a, hipStream_t stream) {
  constexpr int lds = LstmCfg<UP>::kBwdLdsBytes;      // 65 792 bytes at UP = 64: above the 64 KB a launch gets unasked
  TFRS_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(&lstm_bwd_kernel<UP>), lds));
  hipLaunchKernelGGL((lstm_bwd_kernel<UP>), dim3((unsigned)((a.B + 31) / 32)), dim3(LstmCfg<UP>::kWaves * 64), lds,
                     stream, a);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

static int lstm_check_shape(const char *who, int64_t batch, int steps, int units) {
  TFRS_CHECK_ARG(batch >= 0 && steps >= 0 && units >= 1, "%s: bad shape", who);
  if (units > TFRS_LSTM_MAX_UNITS) {
    set_error("%s: units = %d is above the %d the recurrence kernels hold on chip", who, units, TFRS_LSTM_MAX_UNITS);
    return TFRS_ENOTIMPL;
  }
  TFRS_CHECK_ARG(batch <= (int64_t)0x7FFFFFFF * 32, "%s: batch too large", who);
  return TFRS_OK;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_lstm_fwd(const float *xproj, const float *recurrent_kernel, const uint8_t *mask, const float *h0,
                             const float *c0, int64_t batch, int steps, int units, int go_backwards, float *out_seq,
                             float *out_h, float *out_c, float *save_i, float *save_f, float *save_g, float *save_o,
                             float *save_cprev, float *save_hprev, void *stream) {
  const int rc = lstm_check_shape("lstm_fwd", batch, steps, units);
  if (rc != TFRS_OK) return rc;
  if (batch == 0 || steps == 0) return TFRS_OK;
  TFRS_CHECK_ARG(xproj && recurrent_kernel && out_h && out_c, "lstm_fwd: NULL pointer");
  const int nsave = (save_i != nullptr) + (save_f != nullptr) + (save_g != nullptr) + (save_o != nullptr) +
                    (save_cprev != nullptr) + (save_hprev != nullptr);
  TFRS_CHECK_ARG(nsave == 0 || nsave == 6, "lstm_fwd: the six saved tensors come together or not at all");
  LstmFwdArgs a{xproj, recurrent_kernel, mask, h0, c0, batch, steps, units, go_backwards ? 1 : 0, out_seq, out_h,
                out_c, save_i, save_f, save_g, save_o, save_cprev, save_hprev};
  switch (softmax_padded_dim(units)) {
    case 8: return lstm_launch_fwd<8>(a, (hipStream_t)stream);
    case 16: return lstm_launch_fwd<16>(a, (hipStream_t)stream);
    case 32: return lstm_launch_fwd<32>(a, (hipStream_t)stream);
    default: return lstm_launch_fwd<64>(a, (hipStream_t)stream);
  }
}

extern "C" int tfrs_lstm_bwd(const float *recurrent_kernel, const uint8_t *mask, const float *save_i,
                             const float *save_f, const float *save_g, const float *save_o, const float *save_cprev,
                             const float *dseq, const float *dlast_h, const float *dlast_c, int64_t batch, int steps,
                             int units, int go_backwards, float *da, float *dh0, float *dc0, void *stream) {
  const int rc = lstm_check_shape("lstm_bwd", batch, steps, units);
  if (rc != TFRS_OK) return rc;
  if (batch == 0 || steps == 0) return TFRS_OK;
  TFRS_CHECK_ARG(recurrent_kernel && save_i && save_f && save_g && save_o && save_cprev && da && dh0 && dc0,
                 "lstm_bwd: NULL pointer");
  LstmBwdArgs a{recurrent_kernel, mask, save_i, save_f, save_g, save_o, save_cprev, dseq, dlast_h, dlast_c, batch,
                steps, units, go_backwards ? 1 : 0, da, dh0, dc0};
  switch (softmax_padded_dim(units)) {
    case 8: return lstm_launch_bwd<8>(a, (hipStream_t)stream);
    case 16: return lstm_launch_bwd<16>(a, (hipStream_t)stream);
    case 32: return lstm_launch_bwd<32>(a, (hipStream_t)stream);
    default: return lstm_launch_bwd<64>(a, (hipStream_t)stream);
  }
}
