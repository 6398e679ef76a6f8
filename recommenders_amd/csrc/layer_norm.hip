// layer_norm.hip -- LayerNormalization over the last axis of x[N, D], with an optional fused residual add, and its
// backward (layers/layer_norm.py).  All f32, pure HBM kernels: a row is read once, lives in registers
// through both reductions and is written once.
//
//   forward    s = x (+ residual);  mean = sum(s) / D;  var = sum((s - mean)^2) / D  (the two-pass form of
//              tf.nn.moments, on the register copy);  rstd = 1 / sqrt(var + eps)  (IEEE square root and division);
//              y = (s - mean) rstd gamma + beta.  Writes y, optionally s, mean[N] and rstd[N].
//   backward   xhat = (x - mean) rstd;  g = dy gamma;  c1 = mean(g);  c2 = mean(g xhat);
//              dx = rstd (g - c1 - xhat c2) (+ dsum);  dgamma_j = sum_n dy xhat,  dbeta_j = sum_n dy.
//
// Routes.  G lanes share a row and a lane holds K quads (4 K floats) of it:
//   sub-wave     G in {8, 16, 32, 64}, the smallest that holds the row with K <= 4; a wave normalises 64 / G rows at
//                once and the reductions are xor butterflies inside the group, no LDS.
//   workgroup    G = 256 (one row per workgroup), K <= 8; the butterflies end per wave and the four wave sums cross
//                through four floats of LDS, added as (w0 + w1) + (w2 + w3).
//   VEC          D % 4 == 0 and every pointer 16-byte aligned: quad k of lane l is the float4 at column 4 (l + G k), so
//                a group's k-th load covers 16 G contiguous bytes.  Otherwise (dword) element e of lane l is column
//                l + G e.  Either way the reduction order of a row is fixed by (D, alignment) alone.
// Workgroups walk the rows in a grid-stride loop; the grid is min(ceil(N / rows per workgroup),
// TFRS_LAYER_NORM_MAX_GROUPS), a function of (N, D) and never of the device.
//
// dgamma / dbeta without atomics: a lane owns the same columns for every row it visits and accumulates them in
// registers across its loop; at the end the groups of a workgroup add their accumulators through LDS in group order
// and the workgroup writes one slab partial[workgroup][2][D]; a second launch sums the slabs in an order fixed by the
// grid.  The same bits on every run.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace tfrs {

constexpr int kLnThreads = 256;
constexpr int kLnReduceCols = 16, kLnReduceSegs = 16;     // the slab-sum kernel: 16 columns x 16 slab segments

// column of element e (quad e / 4, component e % 4) of lane l
template <bool VEC, int G> __device__ __forceinline__ int ln_col(int l, int e) {
  return VEC ? 4 * (l + G * (e >> 2)) + (e & 3) : l + G * e;
}

// the lane's 4 K elements of the row at p; columns >= d, and every column when p is NULL, read as `fill`
template <bool VEC, int G, int K>
__device__ __forceinline__ void ln_load(float (&v)[4 * K], const float *__restrict__ p, int l, int d, float fill) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (VEC) {
      const int c0 = 4 * (l + G * k);
      float4 t = make_float4(fill, fill, fill, fill);
      if (p != nullptr && c0 < d) t = *reinterpret_cast<const float4 *>(p + c0);
      v[4 * k + 0] = t.x;
      v[4 * k + 1] = t.y;
      v[4 * k + 2] = t.z;
      v[4 * k + 3] = t.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = l + G * (4 * k + c);
        v[4 * k + c] = (p != nullptr && col < d) ? p[col] : fill;
      }
    }
  }
}

template <bool VEC, int G, int K>
__device__ __forceinline__ void ln_store(const float (&v)[4 * K], float *__restrict__ p, int l, int d) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (VEC) {
      const int c0 = 4 * (l + G * k);
      if (c0 < d) *reinterpret_cast<float4 *>(p + c0) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = l + G * (4 * k + c);
        if (col < d) p[col] = v[4 * k + c];
      }
    }
  }
}

// Sum over the G lanes of a row, the same bits in every lane.  Called by all 256 threads of the workgroup.
template <int G> __device__ __forceinline__ float ln_group_sum(float v, float *red) {
  constexpr int W = G < 64 ? G : 64;
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (G == kLnThreads) {
    __syncthreads();        // the previous sum's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (red[0] + red[1]) + (red[2] + red[3]);
  }
  return v;
}

template <bool VEC, int G, int K>
__global__ void __launch_bounds__(kLnThreads)
layer_norm_fwd_kernel(const float *__restrict__ x, const float *__restrict__ residual, const float *__restrict__ gamma,
                      const float *__restrict__ beta, int64_t n, int d, float eps, float *__restrict__ y,
                      float *__restrict__ sum_out, float *__restrict__ mean_out, float *__restrict__ rstd_out) {
  constexpr int E = 4 * K, RPW = kLnThreads / G;
  __shared__ float red[4];
  const int l = threadIdx.x % G, gi = threadIdx.x / G;
  const float fd = (float)d;
  float gm[E], bt[E];
  ln_load<VEC, G, K>(gm, gamma, l, d, 1.0f);
  ln_load<VEC, G, K>(bt, beta, l, d, 0.0f);
  for (int64_t base = (int64_t)blockIdx.x * RPW; base < n; base += (int64_t)gridDim.x * RPW) {
    const int64_t row = base + gi;
    const bool valid = row < n;
    float v[E];
    ln_load<VEC, G, K>(v, valid ? x + row * d : nullptr, l, d, 0.0f);
    if (residual != nullptr) {
      float r[E];
      ln_load<VEC, G, K>(r, valid ? residual + row * d : nullptr, l, d, 0.0f);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] += r[e];
      if (sum_out != nullptr && valid) ln_store<VEC, G, K>(v, sum_out + row * d, l, d);
    }
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += v[e];
    const float mean = ln_group_sum<G>(s, red) / fd;
    float q = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      v[e] = ln_col<VEC, G>(l, e) < d ? v[e] - mean : 0.0f;
      q = fmaf(v[e], v[e], q);
    }
    const float var = ln_group_sum<G>(q, red) / fd;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = fmaf(v[e] * rstd, gm[e], bt[e]);
    if (valid) {
      ln_store<VEC, G, K>(v, y + row * d, l, d);
      if (l == 0) {
        if (mean_out != nullptr) mean_out[row] = mean;
        if (rstd_out != nullptr) rstd_out[row] = rstd;
      }
    }
  }
}

// partial == NULL: no parameter gradient is wanted, nothing is accumulated.  dx == NULL: only the parameter gradients.
template <bool VEC, int G, int K>
__global__ void __launch_bounds__(kLnThreads)
layer_norm_bwd_kernel(const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ rstd,
                      const float *__restrict__ gamma, const float *__restrict__ dy, const float *__restrict__ dsum,
                      int64_t n, int d, float *__restrict__ dx, float *__restrict__ partial) {
  constexpr int E = 4 * K, RPW = kLnThreads / G, NG = RPW;
  __shared__ float red[4];
  __shared__ float acc_lds[NG > 1 ? E * kLnThreads : 1];
  const int l = threadIdx.x % G, gi = threadIdx.x / G;
  const float fd = (float)d;
  float gm[E], acc_g[E], acc_b[E];
  ln_load<VEC, G, K>(gm, gamma, l, d, 1.0f);
#pragma unroll
  for (int e = 0; e < E; ++e) acc_g[e] = acc_b[e] = 0.0f;
  for (int64_t base = (int64_t)blockIdx.x * RPW; base < n; base += (int64_t)gridDim.x * RPW) {
    const int64_t row = base + gi;
    const bool valid = row < n;
    float xh[E], g[E];
    ln_load<VEC, G, K>(xh, valid ? x + row * d : nullptr, l, d, 0.0f);
    ln_load<VEC, G, K>(g, valid ? dy + row * d : nullptr, l, d, 0.0f);
    const float m = valid ? mean[row] : 0.0f, r = valid ? rstd[row] : 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xh[e] = ln_col<VEC, G>(l, e) < d ? (xh[e] - m) * r : 0.0f;
      if (partial != nullptr) {       // dy is zero in columns >= d and in rows >= n
        acc_g[e] = fmaf(g[e], xh[e], acc_g[e]);
        acc_b[e] += g[e];
      }
      g[e] *= gm[e];
      s1 += g[e];
      s2 = fmaf(g[e], xh[e], s2);
    }
    const float c1 = ln_group_sum<G>(s1, red) / fd;
    const float c2 = ln_group_sum<G>(s2, red) / fd;
    if (dx != nullptr) {
#pragma unroll
      for (int e = 0; e < E; ++e) g[e] = r * ((g[e] - c1) - xh[e] * c2);
      if (dsum != nullptr) {
        ln_load<VEC, G, K>(xh, valid ? dsum + row * d : nullptr, l, d, 0.0f);
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] += xh[e];
      }
      if (valid) ln_store<VEC, G, K>(g, dx + row * d, l, d);
    }
  }
  if (partial == nullptr) return;
  float *__restrict__ slab = partial + (int64_t)blockIdx.x * 2 * d;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const float(&acc)[E] = which ? acc_b : acc_g;
    if (NG == 1) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (ln_col<VEC, G>(l, e) < d) slab[which * d + ln_col<VEC, G>(l, e)] = acc[e];
    } else {
      // element e of group gi's lane l sits at acc_lds[e][gi G + l]; group e % NG adds the NG copies in group order
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e) acc_lds[e * kLnThreads + threadIdx.x] = acc[e];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (gi == e % NG && ln_col<VEC, G>(l, e) < d) {
          float t = acc_lds[e * kLnThreads + l];
          for (int o = 1; o < NG; ++o) t += acc_lds[e * kLnThreads + o * G + l];
          slab[which * d + ln_col<VEC, G>(l, e)] = t;
        }
      }
    }
  }
}

// partial[groups][2 d] -> dgamma[d], dbeta[d].  Thread (segment s, column c) adds slabs s, s + 16, ... in that order;
// the 16 segment sums of a column are added in segment order.
__global__ void __launch_bounds__(kLnThreads)
layer_norm_param_sum_kernel(const float *__restrict__ partial, int groups, int d, float *__restrict__ dgamma,
                            float *__restrict__ dbeta) {
  __shared__ float lds[kLnReduceSegs][kLnReduceCols];
  const int c = threadIdx.x % kLnReduceCols, s = threadIdx.x / kLnReduceCols;
  const int j = blockIdx.x * kLnReduceCols + c;
  float t = 0.0f;
  if (j < 2 * d)
    for (int w = s; w < groups; w += kLnReduceSegs) t += partial[(int64_t)w * 2 * d + j];
  lds[s][c] = t;
  __syncthreads();
  if (s == 0 && j < 2 * d) {
    float total = lds[0][c];
#pragma unroll
    for (int o = 1; o < kLnReduceSegs; ++o) total += lds[o][c];
    float *out = j < d ? dgamma : dbeta;
    if (out != nullptr) out[j < d ? j : j - d] = total;
  }
}

struct LnRoute {
  int g, k;       // lanes per row (256: the workgroup route), quads per lane
};
static inline LnRoute ln_route(int64_t d) {
  if (d <= 32) return {8, 1};
  if (d <= 64) return {8, 2};
  if (d <= 128) return {8, 4};
  if (d <= 256) return {16, 4};
  if (d <= 512) return {32, 4};
  if (d <= 1024) return {64, 4};
  if (d <= 2048) return {256, 2};
  if (d <= 4096) return {256, 4};
  return {256, 8};
}
static inline unsigned ln_grid(int64_t n, int64_t d) {
  const int64_t rpw = kLnThreads / ln_route(d).g;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + rpw - 1) / rpw, TFRS_LAYER_NORM_MAX_GROUPS));
}
static inline bool ln_aligned16(std::initializer_list<const void *> ptrs) {
  for (const void *p : ptrs)
    if (((uintptr_t)p) & 15) return false;
  return true;
}

// calls LAUNCH(VEC, G, K) for the route of (d, vec)
#define TFRS_LN_DISPATCH(route, vec, LAUNCH)                              \
  do {                                                                    \
    const int key_ = (route).g * 16 + (route).k;                          \
    switch (key_) {                                                       \
      case 8 * 16 + 1: if (vec) LAUNCH(true, 8, 1); else LAUNCH(false, 8, 1); break;         \
      case 8 * 16 + 2: if (vec) LAUNCH(true, 8, 2); else LAUNCH(false, 8, 2); break;         \
      case 8 * 16 + 4: if (vec) LAUNCH(true, 8, 4); else LAUNCH(false, 8, 4); break;         \
      case 16 * 16 + 4: if (vec) LAUNCH(true, 16, 4); else LAUNCH(false, 16, 4); break;      \
      case 32 * 16 + 4: if (vec) LAUNCH(true, 32, 4); else LAUNCH(false, 32, 4); break;      \
      case 64 * 16 + 4: if (vec) LAUNCH(true, 64, 4); else LAUNCH(false, 64, 4); break;      \
      case 256 * 16 + 2: if (vec) LAUNCH(true, 256, 2); else LAUNCH(false, 256, 2); break;   \
      case 256 * 16 + 4: if (vec) LAUNCH(true, 256, 4); else LAUNCH(false, 256, 4); break;   \
      default: if (vec) LAUNCH(true, 256, 8); else LAUNCH(false, 256, 8); break;             \
    }                                                                     \
  } while (0)

}  // namespace tfrs

using namespace tfrs;

static int ln_check_shape(const char *who, int64_t n, int64_t d) {
  TFRS_CHECK_ARG(n >= 0 && d >= 1, "%s: bad shape (N %lld, D %lld)", who, (long long)n, (long long)d);
  if (d > TFRS_LAYER_NORM_MAX_DIM) {
    set_error("%s: D = %lld is above the %d a workgroup's registers hold", who, (long long)d, TFRS_LAYER_NORM_MAX_DIM);
    return TFRS_ENOTIMPL;
  }
  TFRS_CHECK_ARG(n <= INT64_MAX / d, "%s: N D overflows (N %lld, D %lld)", who, (long long)n, (long long)d);
  return TFRS_OK;
}

extern "C" int tfrs_layer_norm_fwd(const float *x, const float *residual, const float *gamma, const float *beta,
                                   int64_t N, int64_t D, float eps, float *y, float *sum_out, float *mean,
                                   float *rstd, void *stream) {
  const int rc = ln_check_shape("layer_norm_fwd", N, D);
  if (rc != TFRS_OK) return rc;
  if (N == 0) return TFRS_OK;
  TFRS_CHECK_ARG(x && y, "layer_norm_fwd: NULL x or y");
  TFRS_CHECK_ARG(residual || !sum_out, "layer_norm_fwd: sum_out without a residual");
  for (const void *p : {(const void *)x, (const void *)residual, (const void *)gamma, (const void *)beta,
                        (const void *)y, (const void *)sum_out, (const void *)mean, (const void *)rstd})
    TFRS_CHECK_ARG(((uintptr_t)p) % 4 == 0, "layer_norm_fwd: a pointer is not aligned to 4 bytes");
  const bool vec = D % 4 == 0 && ln_aligned16({x, residual, gamma, beta, y, sum_out});
  const LnRoute route = ln_route(D);
  const dim3 grid(ln_grid(N, D)), block(kLnThreads);
  hipStream_t s = (hipStream_t)stream;
#define TFRS_LN_FWD(VEC, G, K)                                                                                   \
  hipLaunchKernelGGL((layer_norm_fwd_kernel<VEC, G, K>), grid, block, 0, s, x, residual, gamma, beta, N, (int)D, \
                     eps, y, sum_out, mean, rstd)
  TFRS_LN_DISPATCH(route, vec, TFRS_LN_FWD);
#undef TFRS_LN_FWD
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" size_t tfrs_layer_norm_workspace_bytes(int64_t N, int64_t D) {
  if (N <= 0 || D < 1 || D > TFRS_LAYER_NORM_MAX_DIM) return 0;
  return (size_t)ln_grid(N, D) * 2 * (size_t)D * sizeof(float);
}

extern "C" int tfrs_layer_norm_bwd(const float *x, const float *mean, const float *rstd, const float *gamma,
                                   const float *dy, const float *dsum, int64_t N, int64_t D, float *dx, float *dgamma,
                                   float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
  const int rc = ln_check_shape("layer_norm_bwd", N, D);
  if (rc != TFRS_OK) return rc;
  if (N == 0) return TFRS_OK;
  const bool params = dgamma != nullptr || dbeta != nullptr;
  TFRS_CHECK_ARG(x && mean && rstd && dy, "layer_norm_bwd: NULL x, mean, rstd or dy");
  TFRS_CHECK_ARG(dx || params, "layer_norm_bwd: no output wanted");
  TFRS_CHECK_ARG(dx || !dsum, "layer_norm_bwd: dsum without dx");
  for (const void *p : {(const void *)x, (const void *)mean, (const void *)rstd, (const void *)gamma,
                        (const void *)dy, (const void *)dsum, (const void *)dx, (const void *)dgamma,
                        (const void *)dbeta, (const void *)workspace})
    TFRS_CHECK_ARG(((uintptr_t)p) % 4 == 0, "layer_norm_bwd: a pointer is not aligned to 4 bytes");
  const size_t need = tfrs_layer_norm_workspace_bytes(N, D);
  TFRS_CHECK_ARG(!params || (workspace && workspace_bytes >= need),
                 "layer_norm_bwd: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need);
  const bool vec = D % 4 == 0 && ln_aligned16({x, gamma, dy, dsum, dx});
  const LnRoute route = ln_route(D);
  const dim3 grid(ln_grid(N, D)), block(kLnThreads);
  float *partial = params ? (float *)workspace : nullptr;
  hipStream_t s = (hipStream_t)stream;
#define TFRS_LN_BWD(VEC, G, K)                                                                                  \
  hipLaunchKernelGGL((layer_norm_bwd_kernel<VEC, G, K>), grid, block, 0, s, x, mean, rstd, gamma, dy, dsum, N, \
                     (int)D, dx, partial)
  TFRS_LN_DISPATCH(route, vec, TFRS_LN_BWD);
#undef TFRS_LN_BWD
  TFRS_LAUNCH_CHECK();
  if (params) {
    const unsigned cols = (unsigned)((2 * D + kLnReduceCols - 1) / kLnReduceCols);
    hipLaunchKernelGGL(layer_norm_param_sum_kernel, dim3(cols), block, 0, s, (const float *)partial, (int)grid.x,
                       (int)D, dgamma, dbeta);
    TFRS_LAUNCH_CHECK();
  }
  return TFRS_OK;
}
