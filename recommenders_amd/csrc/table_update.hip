// The dense halves of the table optimizers: Adagrad (adagrad_dense_multi_kernel) and optimizers.SGD / Adam / Ftrl (the rule
// of table_rules.h as a template parameter) on up to 32 dense tensors per launch, Adam's device-side step counter,
// optimizers.RowWiseAdagrad on a dense 2-D parameter, and the learning-rate schedules every optimizer evaluates on the
// device (lr_tick_kernel).  The sparse-row kernels of the same optimizers live in sparse_update.hip, next to the sort
// and the row scan.
#include "common.h"
#include "table_rules.h"

namespace tfrs {

struct DenseUpdateTensors {
  int ntensors;
  int first_block[33];
  float *p[32];
  float *s0[32];
  float *s1[32];
  const float *g[32];
  int64_t n[32];
};
constexpr int kDenseUpdatePerBlock = 256 * 16;

// tensor t owns blocks [first_block[t], first_block[t + 1]) of 256 threads x 4 x float4; a tensor that is not 16-byte
// aligned, and the block in which a tensor ends, take the scalar loop
template <typename RULE>
__global__ void __launch_bounds__(256) table_update_dense_multi_kernel(const DenseUpdateTensors t, const RULE rule_arg) {
  const RULE rule = rule_arg.resolved();
  int k = 0;
  while (k + 1 < t.ntensors && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
  float *__restrict__ p = t.p[k];
  float *__restrict__ s0 = t.s0[k];
  float *__restrict__ s1 = t.s1[k];
  const float *__restrict__ g = t.g[k];
  const int64_t n = t.n[k];
  const int64_t base = (int64_t)((int)blockIdx.x - t.first_block[k]) * kDenseUpdatePerBlock;
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(s0) | reinterpret_cast<uintptr_t>(s1) |
                     reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  if (vec && base + kDenseUpdatePerBlock <= n) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gv[4], pv[4], av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + (int64_t)(u * 256 + threadIdx.x) * 4;
      gv[u] = *reinterpret_cast<const float4 *>(g + i);
      pv[u] = *reinterpret_cast<const float4 *>(p + i);
      av[u] = RULE::kSlots >= 1 ? *reinterpret_cast<const float4 *>(s0 + i) : zero;
      bv[u] = RULE::kSlots >= 2 ? *reinterpret_cast<const float4 *>(s1 + i) : zero;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + (int64_t)(u * 256 + threadIdx.x) * 4;
      rule.apply(gv[u].x, pv[u].x, av[u].x, bv[u].x);
      rule.apply(gv[u].y, pv[u].y, av[u].y, bv[u].y);
      rule.apply(gv[u].z, pv[u].z, av[u].z, bv[u].z);
      rule.apply(gv[u].w, pv[u].w, av[u].w, bv[u].w);
      *reinterpret_cast<float4 *>(p + i) = pv[u];
      if (RULE::kSlots >= 1) *reinterpret_cast<float4 *>(s0 + i) = av[u];
      if (RULE::kSlots >= 2) *reinterpret_cast<float4 *>(s1 + i) = bv[u];
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < n && i < base + kDenseUpdatePerBlock; i += 256) {
    float w = p[i], a = RULE::kSlots >= 1 ? s0[i] : 0.f, b = RULE::kSlots >= 2 ? s1[i] : 0.f;
    rule.apply(g[i], w, a, b);
    p[i] = w;
    if (RULE::kSlots >= 1) s0[i] = a;
    if (RULE::kSlots >= 2) s1[i] = b;
  }
}

// ---- dense Adagrad of several parameters in ONE launch -------------------------------------------------------------
// The dense parameters of a ranking model (Cross kernels, MLP kernels and biases: 18 tensors at configs[3]) were
// updated by four torch kernels each -- addcmul, add, sqrt, addcdiv: 72 launches and 0.43 ms of a 54 ms step, most of
// them a few KB.  The layout above with s0 the accumulator; same arithmetic as the sparse rows (adagrad_denom):
// acc += g * g; p -= lr * g / denom(acc).
template <typename LR = LrValue>
__global__ void __launch_bounds__(256) adagrad_dense_multi_kernel(const DenseUpdateTensors t, const LR lr_arg, float eps,
                                                                  int mode) {
  const float lr = lr_arg.get();
  int k = 0;
  while (k + 1 < t.ntensors && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
  float *__restrict__ p = t.p[k];
  float *__restrict__ acc = t.s0[k];
  const float *__restrict__ g = t.g[k];
  const int64_t n = t.n[k];
  const int64_t base = (int64_t)((int)blockIdx.x - t.first_block[k]) * kDenseUpdatePerBlock;
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  if (vec && base + kDenseUpdatePerBlock <= n) {
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
      av[u].x += gv[u].x * gv[u].x; av[u].y += gv[u].y * gv[u].y; av[u].z += gv[u].z * gv[u].z; av[u].w += gv[u].w * gv[u].w;
      pv[u].x -= lr * gv[u].x / adagrad_denom(av[u].x, eps, mode);
      pv[u].y -= lr * gv[u].y / adagrad_denom(av[u].y, eps, mode);
      pv[u].z -= lr * gv[u].z / adagrad_denom(av[u].z, eps, mode);
      pv[u].w -= lr * gv[u].w / adagrad_denom(av[u].w, eps, mode);
      *reinterpret_cast<float4 *>(acc + i) = av[u];
      *reinterpret_cast<float4 *>(p + i) = pv[u];
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < n && i < base + kDenseUpdatePerBlock; i += 256) {
    const float gi = g[i];
    const float a = acc[i] + gi * gi;
    acc[i] = a;
    p[i] = p[i] - lr * gi / adagrad_denom(a, eps, mode);
  }
}

// (host) the argument arrays of a dense multi-tensor entry: `nslots` of the slot arrays (0, 1 or 2) are required, the
// others are not read.  dense_update_arrays checks the arrays themselves (an entry's own checks come between the two),
// dense_update_pack the tensors, and fills DenseUpdateTensors and the launch's block count.
static int dense_update_arrays(const char *who, int ntensors, float *const *params_h, float *const *slot0_h,
                               float *const *slot1_h, const float *const *grads_h, const int64_t *n_h, int nslots) {
  TFRS_CHECK_ARG(ntensors >= 1 && ntensors <= 32, "%s: 1..32 tensors", who);
  TFRS_CHECK_ARG(params_h && grads_h && n_h && (nslots < 1 || slot0_h) && (nslots < 2 || slot1_h),
                 "%s: NULL argument array", who);
  return TFRS_OK;
}
static int dense_update_pack(const char *who, int ntensors, float *const *params_h, float *const *slot0_h,
                             float *const *slot1_h, const float *const *grads_h, const int64_t *n_h, int nslots,
                             DenseUpdateTensors *t, int64_t *blocks_out) {
  t->ntensors = ntensors;
  int64_t blocks = 0;
  for (int i = 0; i < ntensors; ++i) {
    TFRS_CHECK_ARG(n_h[i] >= 0 && (n_h[i] == 0 || (params_h[i] && grads_h[i] && (nslots < 1 || slot0_h[i]) &&
                                                   (nslots < 2 || slot1_h[i]))),
                   "%s: bad tensor %d", who, i);
    t->first_block[i] = (int)blocks;
    blocks += (n_h[i] + kDenseUpdatePerBlock - 1) / kDenseUpdatePerBlock;
    TFRS_CHECK_ARG(blocks < (1ll << 31), "%s: too many elements for one launch", who);
    t->p[i] = params_h[i]; t->g[i] = grads_h[i]; t->n[i] = n_h[i];
    t->s0[i] = nslots >= 1 ? slot0_h[i] : nullptr;
    t->s1[i] = nslots >= 2 ? slot1_h[i] : nullptr;
  }
  t->first_block[ntensors] = (int)blocks;
  *blocks_out = blocks;
  return TFRS_OK;
}

template <typename RULE>
static int table_update_dense_launch(const DenseUpdateTensors &t, int64_t blocks, const RULE &rule, hipStream_t s) {
  hipLaunchKernelGGL((table_update_dense_multi_kernel<RULE>), dim3((unsigned)blocks), dim3(256), 0, s, t, rule);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- optimizers.RowWiseAdagrad on a dense 2-D parameter (table_rules.h: one accumulator scalar per row) ------------
// One lane group per row over ALL rows (the group, REREAD and the arithmetic are those of rowwise_adagrad_sorted_kernel
// in sparse_update.hip; the gradient of a chunk is one load).  A row whose gradient is all zero adds 0 to its accumulator and
// scale * 0 to its weights: it keeps its bits.
template <int VEC, bool REREAD, typename LR>
__global__ void __launch_bounds__(256) rowwise_adagrad_dense_kernel(float *__restrict__ param, float *__restrict__ accum,
                                                                    const float *__restrict__ grad, int64_t rows, int d,
                                                                    const LR lr_arg, float eps, int mode,
                                                                    int group_shift) {
  const float lr = lr_arg.get();
  const int per_row = d / VEC;
  const int group = 1 << group_shift;
  const int sub = (int)threadIdx.x & (group - 1);
  const int64_t total = rows << group_shift;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t >> group_shift;      // (uniform over the group)
    const float *__restrict__ grow = grad + r * d;
    auto g_of = [&](int c, float (&g)[VEC]) __attribute__((always_inline)) {
      if (VEC == 4) {
        const float4 e = reinterpret_cast<const float4 *>(grow)[c];
        g[0] = e.x; g[1 % VEC] = e.y; g[2 % VEC] = e.z; g[3 % VEC] = e.w;
      } else {
        g[0] = grow[c];
      }
    };
    rowwise_adagrad_row<VEC, REREAD, false>(sub, group, per_row, d, param + r * d, accum + r, lr, eps, mode, g_of);
  }
}

template <typename LR>
static int rowwise_adagrad_dense_launch(float *param, float *accum, const float *grad, int64_t rows, int d, const LR &lr,
                                        float eps, int mode, hipStream_t s) {
  const bool vec = (d % 4 == 0) && (((uintptr_t)param | (uintptr_t)grad) % 16 == 0);
  const int per_row = vec ? d / 4 : d;
  const int shift = rowwise_group_shift(per_row);
  int64_t blocks = ((rows << shift) + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;     // (grid-stride beyond)
  const dim3 grid((unsigned)blocks), block(256);
#define TFRS_ROWWISE_DENSE(VEC, REREAD) \
  hipLaunchKernelGGL((rowwise_adagrad_dense_kernel<VEC, REREAD, LR>), grid, block, 0, s, param, accum, grad, rows, d, lr, \
                     eps, mode, shift)
  if (vec) {
    if (per_row > 64) TFRS_ROWWISE_DENSE(4, true);
    else TFRS_ROWWISE_DENSE(4, false);
  } else {
    if (per_row > 64) TFRS_ROWWISE_DENSE(1, true);
    else TFRS_ROWWISE_DENSE(1, false);
  }
#undef TFRS_ROWWISE_DENSE
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- learning-rate schedules on the device -------------------------------------------------------------------------
// recommenders_amd/schedules.py describes a schedule as a kind, 8 doubles and an optional f32 table; the kernels below
// evaluate it in float64 at the device counter and round ONCE to f32, so a captured step replays the whole schedule.
//   kind 0  external      lr = table[0] (a device float the user owns, re-read every step)
//        1  exponential   p = {initial, decay_steps, decay_rate, staircase}
//        2  inverse time  p = {initial, decay_steps, decay_rate, staircase}
//        3  polynomial    p = {initial, decay_steps, end, power, cycle}
//        4  cosine        p = {initial, decay_steps, alpha, has_warmup, warmup_target, warmup_steps}
//        5  piecewise     p = boundaries (table_len - 1 of them, at most 7), table = values
//        6  tabulated     table[min(t, table_len - 1)]
enum { kLrExternal = 0, kLrExponential, kLrInverseTime, kLrPolynomial, kLrCosine, kLrPiecewise, kLrTabulated, kLrKinds };

struct LrSchedule {
  int kind;
  double p[8];
  const float *table;
  int64_t table_len;
};

__device__ static float lr_schedule_eval(const LrSchedule &s, int64_t t) {
  if (t < 0) t = 0;
  const double step = (double)t;
  switch (s.kind) {
    case kLrExternal:
      return s.table[0];
    case kLrExponential:
    case kLrInverseTime: {
      double p = step / s.p[1];
      if (s.p[3] != 0.0) p = floor(p);
      return (float)(s.kind == kLrExponential ? s.p[0] * pow(s.p[2], p) : s.p[0] / (1.0 + s.p[2] * p));
    }
    case kLrPolynomial: {
      double x = step, ds = s.p[1];
      if (s.p[4] != 0.0) ds = ds * (t == 0 ? 1.0 : ceil(step / ds));
      else x = fmin(step, ds);
      return (float)((s.p[0] - s.p[2]) * pow(1.0 - x / ds, s.p[3]) + s.p[2]);
    }
    case kLrCosine: {
      double initial = s.p[0], x = step;
      if (s.p[3] != 0.0) {
        if (step < s.p[5]) return (float)(s.p[0] + (s.p[4] - s.p[0]) * step / s.p[5]);
        initial = s.p[4];
        x = step - s.p[5];
      }
      x = fmin(x, s.p[1]);
      const double pi = 3.141592653589793;
      return (float)(initial * ((1.0 - s.p[2]) * 0.5 * (1.0 + cos(pi * x / s.p[1])) + s.p[2]));
    }
    case kLrPiecewise: {
      const int nb = (int)s.table_len - 1;
      for (int i = 0; i < nb; ++i)
        if (step <= s.p[i]) return s.table[i];
      return s.table[nb];
    }
    default:   // kLrTabulated
      return s.table[t < s.table_len - 1 ? t : s.table_len - 1];
  }
}

// One thread: t += advance;  alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t) in float64 from the integer t (powers by
// repeated squaring: at most 2 * 63 products), rounded once to f32.  t is Keras's iterations + 1.
// With lr_out (tfrs_adam_tick_scheduled) the learning rate is the schedule `s` at t - 1 -- Keras's iterations before the
// increment -- rounded to f32 into *lr_out, and alpha is computed from that f32.
__global__ void adam_tick_kernel(int64_t *__restrict__ step, float *__restrict__ alpha, double lr, double beta_1,
                                 double beta_2, int advance, float *__restrict__ lr_out, const LrSchedule s) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t t = *step + advance;
  if (advance) *step = t;
  if (lr_out) {
    const float scheduled = lr_schedule_eval(s, t - 1);
    *lr_out = scheduled;
    lr = (double)scheduled;
  }
  double p1 = 1.0, p2 = 1.0, b1 = beta_1, b2 = beta_2;
  for (int64_t e = t; e > 0; e >>= 1) {
    if (e & 1) {
      p1 *= b1;
      p2 *= b2;
    }
    b1 *= b1;
    b2 *= b2;
  }
  *alpha = (float)(lr * sqrt(1.0 - p2) / (1.0 - p1));
}

// One thread: lr_out[0] = schedule(*iterations); Ftrl also gets lr_out[1] = 2 * (l2 + beta / (2 lr)) from that f32 lr
// (what Ftrl._hyper computes on the host from a float learning rate); then *iterations += advance.
__global__ void lr_tick_kernel(int64_t *__restrict__ iterations, float *__restrict__ lr_out, const LrSchedule s,
                               int ftrl, double l2, double beta, int advance) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t t = *iterations;
  const float lr = lr_schedule_eval(s, t);
  lr_out[0] = lr;
  if (ftrl) lr_out[1] = (float)(2.0 * (l2 + beta / (2.0 * (double)lr)));
  if (advance) *iterations = t + advance;
}

// (before any device call)
static int lr_schedule_check(const char *who, int kind, const double *params_h, const float *table, int64_t table_len,
                             LrSchedule *out) {
  TFRS_CHECK_ARG(kind >= 0 && kind < kLrKinds, "%s: unknown schedule kind %d", who, kind);
  TFRS_CHECK_ARG(params_h, "%s: NULL schedule parameters", who);
  if (kind == kLrExternal || kind == kLrPiecewise || kind == kLrTabulated) {
    TFRS_CHECK_ARG(table && table_len >= 1, "%s: schedule kind %d needs a device table", who, kind);
    TFRS_CHECK_ARG(kind != kLrPiecewise || (table_len >= 2 && table_len <= 8),
                   "%s: a piecewise schedule has 1..7 boundaries and one value more", who);
  }
  if (kind >= kLrExponential && kind <= kLrCosine)
    TFRS_CHECK_ARG(params_h[1] > 0.0, "%s: decay_steps must be positive", who);
  if (kind == kLrCosine && params_h[3] != 0.0)
    TFRS_CHECK_ARG(params_h[5] > 0.0, "%s: warmup_steps must be positive with a warmup_target", who);
  out->kind = kind;
  for (int i = 0; i < 8; ++i) out->p[i] = params_h[i];
  out->table = table;
  out->table_len = table_len;
  return TFRS_OK;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_table_update_dense_multi(int rule, const float *hyper_h, const float *alpha, int ntensors,
                                             float *const *params_h, float *const *slot0_h, float *const *slot1_h,
                                             const float *const *grads_h, const int64_t *n_h, void *stream) {
  int rc = table_rule_check("table_update_dense_multi", rule, hyper_h, alpha);
  if (rc != TFRS_OK) return rc;
  DenseUpdateTensors t = {};
  int64_t blocks = 0;
  const int nslots = rule == kRuleSgd ? 0 : 2;
  rc = dense_update_arrays("table_update_dense_multi", ntensors, params_h, slot0_h, slot1_h, grads_h, n_h, nslots);
  if (rc == TFRS_OK)
    rc = dense_update_pack("table_update_dense_multi", ntensors, params_h, slot0_h, slot1_h, grads_h, n_h, nslots, &t, &blocks);
  if (rc != TFRS_OK) return rc;
  if (blocks == 0) return TFRS_OK;
  hipStream_t s = (hipStream_t)stream;
  // (for SGD and Ftrl a non-NULL alpha is the device floats of tfrs_lr_tick)
  if (rule == kRuleSgd) return table_update_dense_launch(t, blocks, SgdRule{hyper_h[0], alpha}, s);
  if (rule == kRuleAdam) return table_update_dense_launch(t, blocks, AdamRule{hyper_h[0], hyper_h[1], hyper_h[2], alpha}, s);
  if (hyper_h[4] != 0.0f) return table_update_dense_launch(t, blocks, FtrlRule<true>{hyper_h[0], hyper_h[1], hyper_h[2], hyper_h[3], alpha}, s);
  return table_update_dense_launch(t, blocks, FtrlRule<false>{hyper_h[0], hyper_h[1], hyper_h[2], hyper_h[3], alpha}, s);
}

extern "C" int tfrs_adagrad_dense_multi(int ntensors, float *const *params_h, float *const *accum_h,
                                        const float *const *grads_h, const int64_t *n_h, float lr, float eps,
                                        int mode, void *stream) {
  return tfrs_adagrad_dense_multi_dlr(ntensors, params_h, accum_h, grads_h, n_h, lr, nullptr, eps, mode, stream);
}

extern "C" int tfrs_adagrad_dense_multi_dlr(int ntensors, float *const *params_h, float *const *accum_h,
                                            const float *const *grads_h, const int64_t *n_h, float lr,
                                            const float *lr_dev, float eps, int mode, void *stream) {
  DenseUpdateTensors t = {};
  int64_t blocks = 0;
  int rc = dense_update_arrays("adagrad_dense_multi", ntensors, params_h, accum_h, nullptr, grads_h, n_h, 1);
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(mode == 1 || mode == 2, "adagrad_dense_multi: mode must be 1 (sqrt(acc + eps)) or 2 (sqrt(acc) + eps)");
  rc = dense_update_pack("adagrad_dense_multi", ntensors, params_h, accum_h, nullptr, grads_h, n_h, 1, &t, &blocks);
  if (rc != TFRS_OK) return rc;
  if (blocks == 0) return TFRS_OK;
  if (lr_dev)
    hipLaunchKernelGGL(adagrad_dense_multi_kernel<LrDevice>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t,
                       LrDevice{lr_dev}, eps, mode);
  else
    hipLaunchKernelGGL(adagrad_dense_multi_kernel<LrValue>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t,
                       LrValue{lr}, eps, mode);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// (lr_dev: NULL, or the device float of tfrs_lr_tick, read once at kernel entry in place of lr)
extern "C" int tfrs_rowwise_adagrad_dense(float *param, float *accum, const float *grad, int64_t rows, int d, float lr,
                                          const float *lr_dev, float eps, int mode, void *stream) {
  TFRS_CHECK_ARG(mode == 1 || mode == 2, "rowwise_adagrad_dense: mode must be 1 (sqrt(acc + eps)) or 2 (sqrt(acc) + eps)");
  TFRS_CHECK_ARG(rows >= 0 && d >= 1, "rowwise_adagrad_dense: bad shape");
  TFRS_CHECK_ARG(rows < (1ll << 40), "rowwise_adagrad_dense: too many rows");
  TFRS_CHECK_ARG(eps >= 0.f, "rowwise_adagrad_dense: epsilon must be non-negative");
  if (rows == 0) return TFRS_OK;
  TFRS_CHECK_ARG(param && accum && grad, "rowwise_adagrad_dense: NULL pointer");
  if (lr_dev) return rowwise_adagrad_dense_launch(param, accum, grad, rows, d, LrDevice{lr_dev}, eps, mode, (hipStream_t)stream);
  return rowwise_adagrad_dense_launch(param, accum, grad, rows, d, LrValue{lr}, eps, mode, (hipStream_t)stream);
}

extern "C" int tfrs_adam_tick(int64_t *step, float *alpha, double learning_rate, double beta_1, double beta_2,
                              int advance, void *stream) {
  TFRS_CHECK_ARG(step && alpha, "adam_tick: NULL pointer");
  TFRS_CHECK_ARG(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0, "adam_tick: 0 <= beta < 1");
  TFRS_CHECK_ARG(advance == 0 || advance == 1, "adam_tick: advance must be 0 or 1");
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, alpha, learning_rate, beta_1,
                     beta_2, advance, (float *)nullptr, LrSchedule{});
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_lr_tick(int64_t *iterations, float *lr_out, int kind, const double *params_h, const float *table,
                            int64_t table_len, int ftrl, double l2, double beta, int advance, void *stream) {
  TFRS_CHECK_ARG(iterations && lr_out, "lr_tick: NULL pointer");
  TFRS_CHECK_ARG(advance == 0 || advance == 1, "lr_tick: advance must be 0 or 1");
  TFRS_CHECK_ARG(!ftrl || (l2 >= 0.0 && beta >= 0.0), "lr_tick: Ftrl regularizers must be non-negative");
  LrSchedule s;
  int rc = lr_schedule_check("lr_tick", kind, params_h, table, table_len, &s);
  if (rc != TFRS_OK) return rc;
  hipLaunchKernelGGL(lr_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, iterations, lr_out, s, ftrl, l2, beta,
                     advance);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_adam_tick_scheduled(int64_t *step, float *alpha, float *lr_out, int kind, const double *params_h,
                                        const float *table, int64_t table_len, double beta_1, double beta_2,
                                        int advance, void *stream) {
  TFRS_CHECK_ARG(step && alpha && lr_out, "adam_tick_scheduled: NULL pointer");
  TFRS_CHECK_ARG(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0, "adam_tick_scheduled: 0 <= beta < 1");
  TFRS_CHECK_ARG(advance == 0 || advance == 1, "adam_tick_scheduled: advance must be 0 or 1");
  LrSchedule s;
  int rc = lr_schedule_check("adam_tick_scheduled", kind, params_h, table, table_len, &s);
  if (rc != TFRS_OK) return rc;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, alpha, 0.0, beta_1, beta_2,
                     advance, lr_out, s);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
