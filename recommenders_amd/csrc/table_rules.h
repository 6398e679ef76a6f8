// The update rules of optimizers.SGD / Adam / Ftrl as small structs: a slot count (0, 1 or 2 per-element state tensors
// beside the weight) and an `apply` on ONE element.  The three update kernels -- the sorted segments and the row scan of
// embedding.hip, the dense multi-tensor kernel of table_update.hip -- are templates over the rule and are each written
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

namespace tfrs {

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
