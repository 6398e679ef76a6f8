// gru.hip -- the recurrence of a Keras GRU (reset_after=True, tanh / sigmoid, gate order z, r, h) and its
// backward walk, each as ONE launch over all T time steps.
//
//   q   = h_{t-1} @ R + rb                      R = recurrent_kernel [U, 3U], rb = bias[1]
//   z   = sigmoid(a_z + q_z);  r = sigmoid(a_r + q_r);  hh = tanh(a_h + r * q_h)
//   h_t = z * h_{t-1} + (1 - z) * hh            a = x_t @ kernel + bias[0]: a GEMM the caller ran over all t
//   mask[b, t] == 0:  h_t = h_{t-1}
//
// Work mapping: a workgroup owns 32 batch rows (the mfma_tile.h tile) and walks the T steps; wave w owns hidden
// columns [32 w, 32 w + 32) of ALL THREE gates, so z, r, hh and the blend of a column are register arithmetic of the
// lane that holds it (lane = column, 16 accumulator registers = 16 of the 32 rows).  The products run on
// v_mfma_f32_32x32x2_f32 in the half-split k order of mfma_tile.h: A = the h tile (forward) or the gate-gradient
// tile (backward), read from LDS, the only data that crosses waves; B = the wave's slice of R, a register fragment
// read from HBM once per workgroup (3 UP / 2 registers per lane; UP = U padded to 8 / 16 / 32 / 64).
// No atomics, no workspace: every output element is written by exactly one lane.
#include "common.h"
#include "mfma_tile.h"

namespace tfrs {

struct GruFwdArgs {
  const float *xp;        // [B, T, 3U] input projection, bias[0] included
  const float *rk;        // [U, 3U]
  const float *rb;        // [3U] or NULL
  const uint8_t *mask;    // [B, T] or NULL
  const float *h0;        // [B, U] or NULL
  int64_t B;
  int T, U, backwards;
  float *seq;             // [B, T, U] in processing order, or NULL
  float *last;            // [B, U]
  float *sz, *sr, *shh, *sqh, *shp;   // [B, T, U] by time index (training forward), or all NULL
};

struct GruBwdArgs {
  const float *rk;
  const uint8_t *mask;
  const float *sz, *sr, *shh, *sqh, *shp;
  const float *dseq;      // [B, T, U] in processing order, or NULL
  const float *dlast;     // [B, U] or NULL
  int64_t B;
  int T, U, backwards;
  float *da;              // [B, T, 3U]  (da_z, da_r, da_h)
  float *dg;              // [B, T, 3U]  (da_z, da_r, dq_h)
  float *dh0;             // [B, U]
};

__device__ __forceinline__ float gru_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

template <int UP> struct GruCfg {
  static constexpr int kWaves = UP <= 32 ? 1 : UP / 32;
};

// bit i of the result: mask of tile row i at time index tt (all ones without a mask)
__device__ __forceinline__ uint32_t gru_row_mask(const uint8_t *mask, int64_t row0, int64_t B, int T, int tt,
                                                 int jl) {
  if (!mask) return 0xFFFFFFFFu;
  const int64_t row = row0 + jl;
  const bool m = row < B && mask[row * T + tt] != 0;
  return (uint32_t)__ballot(m);
}

template <int UP, bool TRAIN>
__global__ void __launch_bounds__(GruCfg<UP>::kWaves * 64) gru_fwd_kernel(GruFwdArgs a) {
  constexpr int KH = UP / 2, PITCH = UP + 1;
  __shared__ float hs[2][32 * PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int col = wave * 32 + jl;
  const int U = a.U, T = a.T;
  const bool col_ok = col < U;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int64_t ld = 3 * (int64_t)U;

  // B fragment: R[k = hh * KH + s][g * U + col]; zero for padded k and padded columns
  float w[3][KH];
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    const int k = hh * KH + s;
    const bool ok = col_ok && k < U;
#pragma unroll
    for (int g = 0; g < 3; ++g) w[g][s] = ok ? a.rk[k * ld + g * U + col] : 0.0f;
  }
  float rb[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) rb[g] = (a.rb && col_ok) ? a.rb[g * U + col] : 0.0f;

  float h[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int tr = tile_row_of_reg(r, hh);
    const int64_t row = row0 + tr;
    h[r] = (a.h0 && col_ok && row < a.B) ? a.h0[row * U + col] : 0.0f;
    if (col < UP) hs[0][tr * PITCH + col] = h[r];
  }

  for (int t = 0; t < T; ++t) {
    const int tt = a.backwards ? T - 1 - t : t;
    const int cur = t & 1;
    __syncthreads();     // hs[cur] is complete; every wave has finished reading hs[cur ^ 1]
    const uint32_t live = gru_row_mask(a.mask, row0, a.B, T, tt, jl);
    float av[3][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + tile_row_of_reg(r, hh);
      const bool ok = col_ok && row < a.B;
#pragma unroll
      for (int g = 0; g < 3; ++g) av[g][r] = ok ? a.xp[(row * T + tt) * ld + g * U + col] : 0.0f;
    }
    f32x16 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;
    const float *hrow = &hs[cur][jl * PITCH + hh * KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      const float af = hrow[s];
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, w[g][s], acc[g], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = tile_row_of_reg(r, hh);
      const int64_t row = row0 + tr;
      const bool ok = col_ok && row < a.B;
      const float hp = h[r];
      const float qh = acc[2][r] + rb[2];
      const float z = gru_sigmoid(av[0][r] + (acc[0][r] + rb[0]));
      const float rr = gru_sigmoid(av[1][r] + (acc[1][r] + rb[1]));
      const float c = tanhf(av[2][r] + rr * qh);
      const float hn = z * hp + (1.0f - z) * c;
      const float hv = ((live >> tr) & 1u) ? hn : hp;
      h[r] = hv;
      if (ok) {
        if (TRAIN) {
          const int64_t o = (row * T + tt) * U + col;
          a.sz[o] = z;
          a.sr[o] = rr;
          a.shh[o] = c;
          a.sqh[o] = qh;
          a.shp[o] = hp;
        }
        if (a.seq) a.seq[(row * T + t) * U + col] = hv;
      }
      if (col < UP) hs[cur ^ 1][tr * PITCH + col] = col_ok ? hv : 0.0f;
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    if (col_ok && row < a.B) a.last[row * U + col] = h[r];
  }
}

// dh_prev[b][n] = dh[b][n] * z  +  sum_{g, j} dG[b][g][j] * R[n][g U + j]: A = the dG tile [32, 3 UP] through LDS,
// B = row n of R (contiguous in memory), the accumulator starts at dh * z.
template <int UP>
__global__ void __launch_bounds__(GruCfg<UP>::kWaves * 64) gru_bwd_kernel(GruBwdArgs a) {
  constexpr int KH = 3 * UP / 2, PITCH = 3 * UP + 1;
  __shared__ float gs[2][32 * PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jl = lane & 31, hh = lane >> 5;
  const int col = wave * 32 + jl;
  const int U = a.U, T = a.T;
  const bool col_ok = col < U;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int64_t ld = 3 * (int64_t)U;

  // B fragment: k = hh * KH + s = g * UP + j  ->  R[col][g * U + j]
  float w[KH];
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    const int k = hh * KH + s, g = k / UP, j = k % UP;
    w[s] = (col_ok && j < U) ? a.rk[col * ld + g * U + j] : 0.0f;
  }

  float dh[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    dh[r] = (a.dlast && col_ok && row < a.B) ? a.dlast[row * U + col] : 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    const int tt = a.backwards ? T - 1 - t : t;
    const int buf = t & 1;      // two buffers, ONE barrier per step, as the forward's h tile
    const uint32_t live = gru_row_mask(a.mask, row0, a.B, T, tt, jl);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = tile_row_of_reg(r, hh);
      const int64_t row = row0 + tr;
      const bool ok = col_ok && row < a.B;
      const bool on = ok && ((live >> tr) & 1u);
      float d = dh[r];
      float daz = 0.0f, dar = 0.0f, dah = 0.0f, dqh = 0.0f, keep = 1.0f;
      if (ok) {
        if (a.dseq) d += a.dseq[(row * T + t) * U + col];
        if (on) {
          const int64_t o = (row * T + tt) * U + col;
          const float z = a.sz[o], rr = a.sr[o], c = a.shh[o], qh = a.sqh[o], hp = a.shp[o];
          const float dhh = d * (1.0f - z), dz = d * (hp - c);
          dah = dhh * (1.0f - c * c);
          dqh = dah * rr;
          const float dr = dah * qh;
          daz = dz * z * (1.0f - z);
          dar = dr * rr * (1.0f - rr);
          keep = z;
        }
        const int64_t o3 = (row * T + tt) * ld + col;
        a.da[o3] = daz;
        a.da[o3 + U] = dar;
        a.da[o3 + 2 * U] = dah;
        a.dg[o3] = daz;
        a.dg[o3 + U] = dar;
        a.dg[o3 + 2 * U] = dqh;
      }
      acc[r] = on ? d * keep : d;
      if (col < UP) {
        float *grow = &gs[buf][tr * PITCH + col];
        grow[0] = daz;
        grow[UP] = dar;
        grow[2 * UP] = dqh;
      }
    }
    __syncthreads();
    const float *grow = &gs[buf][jl * PITCH + hh * KH];
#pragma unroll
    for (int s = 0; s < KH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[s], w[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = acc[r];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + tile_row_of_reg(r, hh);
    if (col_ok && row < a.B) a.dh0[row * U + col] = dh[r];
  }
}

template <int UP>
static int gru_launch_fwd(const GruFwdArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.B + 31) / 32)), block(GruCfg<UP>::kWaves * 64);
  if (a.sz)
    hipLaunchKernelGGL((gru_fwd_kernel<UP, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((gru_fwd_kernel<UP, false>), grid, block, 0, stream, a);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

template <int UP>
static int gru_launch_bwd(const GruBwdArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL((gru_bwd_kernel<UP>), dim3((unsigned)((a.B + 31) / 32)), dim3(GruCfg<UP>::kWaves * 64), 0,
                     stream, a);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

static int gru_check_shape(const char *who, int64_t batch, int steps, int units) {
  TFRS_CHECK_ARG(batch >= 0 && steps >= 0 && units >= 1, "%s: bad shape", who);
  if (units > TFRS_GRU_MAX_UNITS) {
    set_error("%s: units = %d is above the %d the recurrence kernels hold on chip", who, units, TFRS_GRU_MAX_UNITS);
    return TFRS_ENOTIMPL;
  }
  TFRS_CHECK_ARG(batch <= (int64_t)0x7FFFFFFF * 32, "%s: batch too large", who);
  return TFRS_OK;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_gru_fwd(const float *xproj, const float *recurrent_kernel, const float *recurrent_bias,
                            const uint8_t *mask, const float *h0, int64_t batch, int steps, int units,
                            int go_backwards, float *out_seq, float *out_last, float *save_z, float *save_r,
                            float *save_hh, float *save_qh, float *save_hprev, void *stream) {
  const int rc = gru_check_shape("gru_fwd", batch, steps, units);
  if (rc != TFRS_OK) return rc;
  if (batch == 0 || steps == 0) return TFRS_OK;
  TFRS_CHECK_ARG(xproj && recurrent_kernel && out_last, "gru_fwd: NULL pointer");
  const int nsave = (save_z != nullptr) + (save_r != nullptr) + (save_hh != nullptr) + (save_qh != nullptr) +
                    (save_hprev != nullptr);
  TFRS_CHECK_ARG(nsave == 0 || nsave == 5, "gru_fwd: the five saved tensors come together or not at all");
  GruFwdArgs a{xproj, recurrent_kernel, recurrent_bias, mask, h0, batch, steps, units, go_backwards ? 1 : 0,
               out_seq, out_last, save_z, save_r, save_hh, save_qh, save_hprev};
  switch (softmax_padded_dim(units)) {
    case 8: return gru_launch_fwd<8>(a, (hipStream_t)stream);
    case 16: return gru_launch_fwd<16>(a, (hipStream_t)stream);
    case 32: return gru_launch_fwd<32>(a, (hipStream_t)stream);
    default: return gru_launch_fwd<64>(a, (hipStream_t)stream);
  }
}

extern "C" int tfrs_gru_bwd(const float *recurrent_kernel, const uint8_t *mask, const float *save_z,
                            const float *save_r, const float *save_hh, const float *save_qh,
                            const float *save_hprev, const float *dseq, const float *dlast, int64_t batch,
                            int steps, int units, int go_backwards, float *da, float *dg, float *dh0,
                            void *stream) {
  const int rc = gru_check_shape("gru_bwd", batch, steps, units);
  if (rc != TFRS_OK) return rc;
  if (batch == 0 || steps == 0) return TFRS_OK;
  TFRS_CHECK_ARG(recurrent_kernel && save_z && save_r && save_hh && save_qh && save_hprev && da && dg && dh0,
                 "gru_bwd: NULL pointer");
  GruBwdArgs a{recurrent_kernel, mask, save_z, save_r, save_hh, save_qh, save_hprev, dseq, dlast, batch, steps,
               units, go_backwards ? 1 : 0, da, dg, dh0};
  switch (softmax_padded_dim(units)) {
    case 8: return gru_launch_bwd<8>(a, (hipStream_t)stream);
    case 16: return gru_launch_bwd<16>(a, (hipStream_t)stream);
    case 32: return gru_launch_bwd<32>(a, (hipStream_t)stream);
    default: return gru_launch_bwd<64>(a, (hipStream_t)stream);
  }
}
