// The update rules of optimizers.SGD / Adam / Ftrl as small structs: a slot count (0, 1 or 2 per-element state tensors
// beside the weight) and an `apply` on ONE element.  The three update kernels -- the sorted segments and the row scan of
// sparse_update.hip, the dense multi-tensor kernel of table_update.hip -- are templates over the rule and are each written
// once.  Hyper-parameters travel by value inside the rule; Adam's bias-corrected step size is read from a device float
// that adam_tick_kernel (table_update.hip) writes at the head of every step, so a captured step replays with a live t.
//
// All arithmetic is f32 in exactly the written order: contraction is switched off inside every apply, so a product and
// the sum that follows it round separately, as in the NumPy float32 restatement of tests/table_optimizers_restatement.py.
// Division and sqrtf are correctly rounded (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the build passes
// no fast-math flag).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "row_access.h"

namespace tfrs {

// Denominator of the fused Adagrad update (the sparse kernels of sparse_update.hip, adagrad_dense_multi_kernel of
// table_update.hip; Adagrad is not a rule below: its arithmetic is compiled with contraction on).  adagrad == 1:
// sqrt(acc + eps), tf.keras.optimizers.Adagrad of TF >= 2.11 / tf-keras (`variable.assign_sub(lr * grad /
// sqrt(accumulator + epsilon))`); adagrad == 2: sqrt(acc) + eps, the optimizer_v2 / ResourceApplyAdagradV2 form of
// TF <= 2.10 (the reference's release script pins TF 2.9.0, tools/build_scripts/release.sh:6) -- also
// torch.optim.Adagrad's, which the tests cross-check it against.
__device__ __forceinline__ float adagrad_denom(float acc, float eps, int adagrad) {
  return adagrad == 2 ? sqrtf(acc) + eps : sqrtf(acc + eps);
}

// (the `rule` argument of the C entries)
enum { kRuleSgd = 0, kRuleAdam = 1, kRuleFtrl = 2 };

// How a kernel of the Adagrad update that used to take `float lr` by value gets its learning rate: by value (a constant float
// learning_rate: the same kernel argument bytes and the same code as before), or from a device float that
// lr_tick_kernel (table_update.hip) writes at the head of every step -- one wave-uniform read at kernel entry, so a
// captured step replays a whole schedule.  The kernels are templates over the two, so the constant path keeps its own
// instantiations.
struct LrValue {
  float v;
  __device__ __forceinline__ float get() const { return v; }
};
struct LrDevice {
  const float *p;
  __device__ __forceinline__ float get() const { return *p; }
};

// A rule's `resolved()` is taken ONCE at kernel entry: SGD and Ftrl then read their learning rate from the device floats
// of tfrs_lr_tick when `dev` is set (one wave-uniform read), and are the by-value rule otherwise -- the same
// instantiations serve both, and `apply` below is the only arithmetic.

// tf.keras.optimizers.SGD without momentum:  w -= lr * g
struct SgdRule {
  static constexpr int kSlots = 0;
  float lr;
  const float *dev;     // NULL, or {lr} on the device
  __device__ __forceinline__ SgdRule resolved() const { return SgdRule{dev ? dev[0] : lr, nullptr}; }
  __device__ __forceinline__ void apply(float g, float &w, float &, float &) const {
#pragma clang fp contract(off)
    w = w - lr * g;
  }
};

// tf.keras.optimizers.Adam (slots m, v), alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t) from the device:
//   m += (g - m) * (1 - beta_1);  v += (g * g - v) * (1 - beta_2);  w -= m * alpha / (sqrt(v) + epsilon)
struct AdamRule {
  static constexpr int kSlots = 2;
  float one_minus_beta_1, one_minus_beta_2, epsilon;
  const float *alpha;
  __device__ __forceinline__ AdamRule resolved() const { return *this; }
  __device__ __forceinline__ void apply(float g, float &w, float &m, float &v) const {
#pragma clang fp contract(off)
    const float a = *alpha;
    m = m + (g - m) * one_minus_beta_1;
    v = v + (g * g - v) * one_minus_beta_2;
    w = w - m * a / (sqrtf(v) + epsilon);
  }
};

// tf.keras.optimizers.Ftrl (slots n = accumulator, lin = linear); SQRT: learning_rate_power -0.5 (n^p = sqrt n), else 0
// (n^p = 1).  two_l2r = 2 * (l2 + beta / (2 lr)), two_shrink = 2 * l2_shrinkage:
//   g' = g + 2 shrink w;  n' = n + g * g;  lin += g' - (n'^p - n^p) / lr * w;  q = n'^p / lr + 2 l2r;
//   w = (clip(lin, -l1, l1) - lin) / q;  n = n'
template <bool SQRT>
struct FtrlRule {
  static constexpr int kSlots = 2;
  float lr, l1, two_l2r, two_shrink;
  const float *dev;     // NULL, or {lr, two_l2r} on the device
  __device__ __forceinline__ FtrlRule resolved() const {
    return FtrlRule{dev ? dev[0] : lr, l1, dev ? dev[1] : two_l2r, two_shrink, nullptr};
  }
  __device__ __forceinline__ void apply(float g, float &w, float &n, float &lin) const {
#pragma clang fp contract(off)
    const float gp = g + two_shrink * w;
    const float n2 = n + g * g;
    const float pn2 = SQRT ? sqrtf(n2) : 1.0f;
    const float pn = SQRT ? sqrtf(n) : 1.0f;
    lin = lin + (gp - (pn2 - pn) / lr * w);
    const float q = pn2 / lr + two_l2r;
    w = (fminf(fmaxf(lin, -l1), l1) - lin) / q;
    n = n2;
  }
};

// ---- optimizers.RowWiseAdagrad: ONE accumulator scalar per table row ("exact row-wise Adagrad") ---------------------
// G = the row's summed gradient (duplicates summed first, the bits of the other optimizers' sums), d = the row width:
//   s = (sum_j G_j * G_j) / d;  acc' = acc + s;  den = sqrt(acc' + eps)   (mode 2, legacy: sqrt(acc') + eps)
//   scale = lr / den  (ONE division per row);  w_j' = w_j - scale * G_j
// A rule of the kind above cannot express it (apply sees one element), so it has kernels of its own
// (rowwise_adagrad_sorted_kernel and rowscan_rowwise, the row scan's epilogue, in sparse_update.hip, rowwise_adagrad_dense_kernel
// in table_update.hip); the arithmetic is the four functions below, contraction off as in every rule.
//
// The order of the d additions of sum_j is fixed, so a step is bit-reproducible:
//   sorted route / dense kernel (rowwise_adagrad_row): a row belongs to a group of L lanes, L the power of two
//     >= ceil(d / VEC) and at most 64 (VEC = 4 on the float4 path, else 1).  Lane l of the group owns the VEC-wide chunks
//     l, l + L, l + 2 L, ... of the row and adds their squares to a lane-local partial that starts at +0, chunks in
//     ascending order, the VEC elements of a chunk in ascending order (a lane without a chunk keeps +0); the L partials
//     are then summed by an xor butterfly with the offsets L / 2, L / 4, ..., 1 (x += x of lane ^ offset: every lane ends
//     with the same bits).
//   row scan (a wave per row): lane l owns the features l, l + 64, l + 128, l + 192, ascending, then the same butterfly
//     over 64 lanes.
// The float4 order differs from the row scan's (by float32 reassociation of non-negative terms only); with VEC = 1 a
// chunk is a feature, lane l owns l, l + 64, ... on both routes and a lane without a feature adds +0, so the two are
// the same sum (tests/optimizer_handbuilt.py restates both).  Which route a table takes is a function of (vocab, n, d)
// alone.
__device__ __forceinline__ float rowwise_sq_add(float partial, float g) {
#pragma clang fp contract(off)
  return partial + g * g;
}
__device__ __forceinline__ float rowwise_group_sum(float x, int group) {
  for (int o = group >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);     // (lane ^ o stays inside the aligned group)
  return x;
}
// acc' from the row's sum of squares
__device__ __forceinline__ float rowwise_accumulate(float acc, float sum_sq, int d) {
#pragma clang fp contract(off)
  return acc + sum_sq / (float)d;
}
__device__ __forceinline__ float rowwise_scale(float acc_new, float lr, float eps, int mode) {
#pragma clang fp contract(off)
  const float den = mode == 2 ? sqrtf(acc_new) + eps : sqrtf(acc_new + eps);
  return lr / den;
}
__device__ __forceinline__ float rowwise_step(float w, float scale, float g) {
#pragma clang fp contract(off)
  return w - scale * g;
}

// One row on its lane group (every lane of the group calls this together; `sub` = the lane's index in the group):
// grad(c, g) yields the VEC summed gradients of chunk c.  REREAD = false: ceil(d / VEC) <= group, a lane keeps its one
// chunk of G in registers -- the gradient and the weights are read once.  REREAD = true (wider rows: d > 256 on the
// float4 path, d > 64 on the scalar path): a lane walks its chunks twice, once for the squares and once for the step, so
// the gradient is read (and summed) a second time, bit for bit as the first time; the weights are still read once.
// One lane reads and writes *acc and divides; NT: the row's weights carry the non-temporal hint.
template <int VEC, bool REREAD, bool NT, typename GradFn>
__device__ __forceinline__ void rowwise_adagrad_row(int sub, int group, int per_row, int d, float *__restrict__ wrow,
                                                    float *__restrict__ acc, float lr, float eps, int mode,
                                                    GradFn grad) {
  auto load_w = [&](int c, float (&r)[VEC]) __attribute__((always_inline)) { vec_load<VEC, NT>(wrow + c * VEC, r); };
  auto store_w = [&](int c, const float (&r)[VEC]) __attribute__((always_inline)) { vec_store<VEC, NT>(wrow + c * VEC, r); };
  const bool on = sub < per_row;
  const float a_old = sub == 0 ? *acc : 0.f;
  float g[VEC], w[VEC];
  float partial = 0.f;
  if (!REREAD) {
    if (on) {
      load_w(sub, w);
      grad(sub, g);
#pragma unroll
      for (int v = 0; v < VEC; ++v) partial = rowwise_sq_add(partial, g[v]);
    }
  } else {
    for (int c = sub; c < per_row; c += group) {
      grad(c, g);
#pragma unroll
      for (int v = 0; v < VEC; ++v) partial = rowwise_sq_add(partial, g[v]);
    }
  }
  const float sum_sq = rowwise_group_sum(partial, group);
  float scale = 0.f;
  if (sub == 0) {
    const float a_new = rowwise_accumulate(a_old, sum_sq, d);
    *acc = a_new;
    scale = rowwise_scale(a_new, lr, eps, mode);
  }
  scale = __shfl(scale, (int)(threadIdx.x & 63u) - sub);
  if (!REREAD) {
    if (on) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) w[v] = rowwise_step(w[v], scale, g[v]);
      store_w(sub, w);
    }
  } else {
    for (int c = sub; c < per_row; c += group) {
      load_w(c, w);
      grad(c, g);
#pragma unroll
      for (int v = 0; v < VEC; ++v) w[v] = rowwise_step(w[v], scale, g[v]);
      store_w(c, w);
    }
  }
}

// (host) the lane group of a row of `per_row` chunks: the power of two >= per_row, at most 64; returns its log2
inline int rowwise_group_shift(int64_t per_row) {
  int shift = 0;
  while (shift < 6 && (1ll << shift) < per_row) ++shift;
  return shift;
}

// The argument checks the C entries share (before any device call).  hyper_h, a HOST array of 8 floats:
//   SGD   {lr}
//   Adam  {1 - beta_1, 1 - beta_2, epsilon}, alpha = the device float of tfrs_adam_tick
//   Ftrl  {lr, l1, 2 * (l2 + beta / (2 lr)), 2 * l2_shrinkage, learning_rate_power (-0.5 or 0)}
// For SGD and Ftrl a non-NULL `alpha` is the device floats of tfrs_lr_tick ({lr} / {lr, 2 * l2r}); hyper_h[0] (and
// Ftrl's hyper_h[2]) are then not read.
inline int table_rule_check(const char *who, int rule, const float *h, const float *alpha) {
  TFRS_CHECK_ARG(rule == kRuleSgd || rule == kRuleAdam || rule == kRuleFtrl, "%s: rule must be 0 (SGD), 1 (Adam) or 2 (Ftrl)", who);
  TFRS_CHECK_ARG(h, "%s: NULL hyper-parameters", who);
  if (rule == kRuleSgd && !alpha) TFRS_CHECK_ARG(h[0] == h[0], "%s: SGD learning rate is NaN", who);
  if (rule == kRuleAdam) {
    TFRS_CHECK_ARG(alpha, "%s: Adam needs the device step size of tfrs_adam_tick", who);
    TFRS_CHECK_ARG(h[0] > 0.f && h[0] <= 1.f && h[1] > 0.f && h[1] <= 1.f, "%s: Adam needs 0 <= beta < 1", who);
    TFRS_CHECK_ARG(h[2] >= 0.f, "%s: Adam epsilon must be non-negative", who);
  }
  if (rule == kRuleFtrl) {
    TFRS_CHECK_ARG(alpha || h[0] > 0.f, "%s: Ftrl learning rate must be positive", who);
    TFRS_CHECK_ARG(h[1] >= 0.f && (alpha || h[2] >= 0.f) && h[3] >= 0.f, "%s: Ftrl regularizers must be non-negative", who);
    TFRS_CHECK_ARG(h[4] == -0.5f || h[4] == 0.0f, "%s: Ftrl learning_rate_power must be -0.5 or 0", who);
  }
  return TFRS_OK;
}

}  // namespace tfrs
