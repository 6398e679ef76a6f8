// tfrs_clippy_dense_multi: ClippyAdagrad (experimental/optimizers/clippy_adagrad.py:188-254) on up to 32 dense tensors
// per call -- the Cross / MLP kernels and biases of a ranking model.  See clippy.h for the two-pass scheme; the sparse
// rows of embedding tables are handled next to the radix sort in sparse_update.hip (tfrs_clippy_sparse).
//
// Traffic: the factor pass reads w, acc, g (12 B / element), the apply pass reads them again and writes w, acc
// (20 B / element): 32 B against the 20 B of tfrs_adagrad_dense_multi.  Tensor t owns blocks
// [first_block[t], first_block[t + 1]) of 256 threads x 4 x float4 in both passes, like adagrad_dense_multi_kernel.
#include "common.h"
#include "clippy.h"

namespace tfrs {

struct ClippyDenseTensors {
  int ntensors;
  int first_block[33];
  float *p[32];
  float *acc[32];
  const float *g[32];
  int64_t n[32];
};
constexpr int kClippyPerBlock = 256 * 16;

template <bool APPLY, typename HYPER = ClippyHyper>
__global__ void __launch_bounds__(256) clippy_dense_multi_kernel(const ClippyDenseTensors t, float *__restrict__ factors,
                                                                 const HYPER h_arg) {
  const ClippyHyper h = h_arg.get();
  int k = 0;
  while (k + 1 < t.ntensors && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
  float *__restrict__ p = t.p[k];
  float *__restrict__ acc = t.acc[k];
  const float *__restrict__ g = t.g[k];
  const int64_t n = t.n[k];
  const int64_t base = (int64_t)((int)blockIdx.x - t.first_block[k]) * kClippyPerBlock;
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const float factor = APPLY ? factors[k] : 1.0f;
  float m = 1.0f;
  if (vec && base + kClippyPerBlock <= n) {
    float4 gv[4], av[4], pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + (int64_t)(u * 256 + threadIdx.x) * 4;
      gv[u] = *reinterpret_cast<const float4 *>(g + i);
      av[u] = *reinterpret_cast<const float4 *>(acc + i);
      pv[u] = *reinterpret_cast<const float4 *>(p + i);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + (int64_t)(u * 256 + threadIdx.x) * 4;
      float *gx = &gv[u].x, *ax = &av[u].x, *px = &pv[u].x;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const ClippyElement e = clippy_element(px[c], ax[c], gx[c], h);
        if (APPLY) clippy_apply(e, gx[c], factor, h, px[c], ax[c]);
        else m = clippy_min_scale(m, e);
      }
      if (APPLY) {
        *reinterpret_cast<float4 *>(acc + i) = av[u];
        *reinterpret_cast<float4 *>(p + i) = pv[u];
      }
    }
  } else {
    for (int64_t i = base + threadIdx.x; i < n && i < base + kClippyPerBlock; i += 256) {
      const float gi = g[i];
      float w = p[i], a = acc[i];
      const ClippyElement e = clippy_element(w, a, gi, h);
      if (APPLY) {
        clippy_apply(e, gi, factor, h, w, a);
        acc[i] = a;
        p[i] = w;
      } else {
        m = clippy_min_scale(m, e);
      }
    }
  }
  if (!APPLY) {
    __shared__ float s_min[4];
    m = clippy_wave_min(m);
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
      clippy_factor_min(factors + k, fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3])));
  }
}

}  // namespace tfrs

extern "C" int tfrs_clippy_dense_multi(int ntensors, float *const *params_h, float *const *accum_h,
                                       const float *const *grads_h, const int64_t *n_h, float *factors, float lr,
                                       float eps, float var_rel, float acc_rel, float abs_thr, int mode,
                                       void *stream) {
  return tfrs_clippy_dense_multi_dlr(ntensors, params_h, accum_h, grads_h, n_h, factors, lr, nullptr, eps, var_rel,
                                     acc_rel, abs_thr, mode, stream);
}

// (lr_dev: NULL, or the device float of tfrs_lr_tick, read by both passes in place of lr)
extern "C" int tfrs_clippy_dense_multi_dlr(int ntensors, float *const *params_h, float *const *accum_h,
                                           const float *const *grads_h, const int64_t *n_h, float *factors, float lr,
                                           const float *lr_dev, float eps, float var_rel, float acc_rel, float abs_thr,
                                           int mode, void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(ntensors >= 1 && ntensors <= 32, "clippy_dense_multi: 1..32 tensors");
  TFRS_CHECK_ARG(params_h && accum_h && grads_h && n_h && factors, "clippy_dense_multi: NULL argument");
  TFRS_CHECK_ARG(mode >= 0 && mode <= 2, "clippy_dense_multi: mode must be 0 (delayed), 1 (delayed, clipped) or 2 (standard)");
  TFRS_CHECK_ARG(var_rel >= 0.f && acc_rel >= 0.f && abs_thr >= 0.f, "clippy_dense_multi: thresholds must be non-negative");
  ClippyDenseTensors t = {};
  t.ntensors = ntensors;
  int64_t blocks = 0;
  for (int i = 0; i < ntensors; ++i) {
    TFRS_CHECK_ARG(n_h[i] >= 0 && (n_h[i] == 0 || (params_h[i] && accum_h[i] && grads_h[i])),
                   "clippy_dense_multi: bad tensor %d", i);
    t.first_block[i] = (int)blocks;
    blocks += (n_h[i] + kClippyPerBlock - 1) / kClippyPerBlock;
    TFRS_CHECK_ARG(blocks < (1ll << 31), "clippy_dense_multi: too many elements for one launch");
    t.p[i] = params_h[i]; t.acc[i] = accum_h[i]; t.g[i] = grads_h[i]; t.n[i] = n_h[i];
  }
  t.first_block[ntensors] = (int)blocks;
  const ClippyHyper h = {lr, eps, var_rel, acc_rel, abs_thr, mode};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clippy_arm_kernel, dim3(1), dim3(64), 0, s, factors, ntensors);
  if (blocks > 0 && lr_dev) {
    const ClippyHyperDevice hd = {h, lr_dev};
    hipLaunchKernelGGL((clippy_dense_multi_kernel<false, ClippyHyperDevice>), dim3((unsigned)blocks), dim3(256), 0, s, t, factors, hd);
    hipLaunchKernelGGL((clippy_dense_multi_kernel<true, ClippyHyperDevice>), dim3((unsigned)blocks), dim3(256), 0, s, t, factors, hd);
  } else if (blocks > 0) {
    hipLaunchKernelGGL((clippy_dense_multi_kernel<false, ClippyHyper>), dim3((unsigned)blocks), dim3(256), 0, s, t, factors, h);
    hipLaunchKernelGGL((clippy_dense_multi_kernel<true, ClippyHyper>), dim3((unsigned)blocks), dim3(256), 0, s, t, factors, h);
  }
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
