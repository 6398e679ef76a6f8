// ClippyAdagrad (experimental/optimizers/clippy_adagrad.py:188-254 with shrink_by_references, :21-70) -- the element
// arithmetic shared by the dense kernels (clippy.hip) and the sparse-row kernels (sparse_update.hip, next to the sort).
//
// A variable's clipping factor is a min over the whole variable (or over its touched rows) and has to be known before
// any element is written, so every update is two passes over the same data: a FACTOR pass (reads only; wave / block
// min, then atomicMin on the bit pattern of the non-negative float -- the mirror of the atomicMax-on-float-bits idiom
// of topk_pack.hip / gemm16.hip) and an APPLY pass.  Both go through clippy_element() below, so the factor is exact
// for the very delta that is applied; the accumulator pre-update and the clipped post-update are explicit fmaf()s so
// that no contraction choice can differ between the two passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfrs {

// mode 0: delayed accumulator update (acc += g^2 after the step); 1: delayed and clipped (acc += (g * factor)^2);
// 2: use_standard_accumulator_update (acc += g^2 first, the classical Adagrad order)
struct ClippyHyper {
  float lr, eps, var_rel, acc_rel, abs_thr;
  int mode;
  __device__ __forceinline__ ClippyHyper get() const { return *this; }
};

// ClippyHyper whose lr is read (once, at kernel entry) from the device float of tfrs_lr_tick: the kernels are templates
// over the two, so a constant float learning rate keeps its own instantiations
struct ClippyHyperDevice {
  ClippyHyper h;
  const float *lr;
  __device__ __forceinline__ ClippyHyper get() const {
    ClippyHyper r = h;
    r.lr = *lr;
    return r;
  }
};

struct ClippyElement {
  float acc;     // the accumulator the preconditioner was taken from (mode 2: already + g^2)
  float delta;   // lr * g / sqrt(acc + eps), unclipped
  float maxd;    // |w| * var_rel + acc_rel / sqrt(acc + eps) + abs_thr
};

__device__ __forceinline__ ClippyElement clippy_element(float w, float acc, float g, const ClippyHyper &h) {
  ClippyElement e;
  e.acc = h.mode == 2 ? fmaf(g, g, acc) : acc;
  const float pre = 1.0f / sqrtf(e.acc + h.eps);
  e.delta = h.lr * g * pre;
  {
    // two products and two sums, each rounded on its own: what every Clippy kernel had compiled to while the choice
    // was the compiler's; pinned, because the factor scales every touched row and a reshaped kernel flipped the choice
#pragma clang fp contract(off)
    e.maxd = fabsf(w) * h.var_rel + pre * h.acc_rel + h.abs_thr;
  }
  return e;
}

// m = min(m, largest scale with scale * |delta| <= maxd) (shrink_by_references: 1 where delta == 0; never negative).
// Only a quotient below 1 can lower a min that starts at 1, and maxd / |delta| < 1 exactly when |delta| > maxd, so the
// division runs for the clipped elements only: one IEEE division less per element in the factor pass.
__device__ __forceinline__ float clippy_min_scale(float m, const ClippyElement &e) {
  const float ad = fabsf(e.delta);
  return ad > e.maxd ? fminf(m, e.maxd / ad) : m;
}

// the element's new weight and accumulator under the variable's factor
__device__ __forceinline__ void clippy_apply(const ClippyElement &e, float g, float factor, const ClippyHyper &h,
                                             float &w, float &acc) {
  w = w - e.delta * factor;
  if (h.mode == 2) {
    acc = e.acc;
  } else {
    const float u = h.mode == 1 ? g * factor : g;
    acc = fmaf(u, u, e.acc);
  }
}

__device__ __forceinline__ float clippy_wave_min(float m) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fminf(m, __shfl_xor(m, off));
  return m;
}

// factor = min(factor, m) for m >= 0: non-negative floats order like their bit patterns.  The slot holds 1.0f when
// the pass starts (clippy_arm_kernel), so anything >= 1 needs no atomic.  Min is order-independent: bit-reproducible.
__device__ __forceinline__ void clippy_factor_min(float *factor, float m) {
  if (m < 1.0f) atomicMin(reinterpret_cast<unsigned int *>(factor), __float_as_uint(m));
}

static __global__ void clippy_arm_kernel(float *__restrict__ factors, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) factors[i] = 1.0f;
}

}  // namespace tfrs
