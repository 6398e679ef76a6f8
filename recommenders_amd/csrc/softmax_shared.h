// softmax_shared.h -- what the in-batch softmax translation units share (softmax.hip: the f32-MFMA loss kernels;
// softmax_mined.hip: the same loss over a mined / adjusted kept set): the kernel argument block, the logit
// function, the split planner (TFRS_SOFTMAX_WAVES), the finalize and partial-gradient reduce kernels and their
// launchers.  Kernels and helpers are `static`: each translation unit carries its own copy, nothing is exported.
#pragma once

#include <algorithm>
#include <type_traits>

#include <stdlib.h>

#include "mfma_tile.h"

namespace tfrs {

constexpr float kMinFloat = -3.4028234663852886e36f;  // np.finfo(float32).min / 100

struct SoftmaxArgs {
  const float *q, *c;
  int64_t nq, nc;
  int d;
  const float *w;       // [nq] sample weights or NULL
  float inv_t;          // 1 / temperature
  const float *corr;    // [nc] log(clip(p, 1e-6, 1)) or NULL
  const int64_t *ids;   // [nc] candidate ids (accidental-hit removal) or NULL
  const uint8_t *mask;  // [nq, nc] score_mask or NULL
  int nsplit;
  int64_t split_len;    // multiple of 32
  float *pm, *pl;       // [nsplit, nq] partial max / sum-exp
  float *ppos;          // [nq] positive logit
  const float *lse;     // [nq]
  const float *gloss;   // device scalar or NULL (= 1)
  float *partial;       // [nsplit, rows, d] partial gradients
  uint32_t *ticket;     // finalize kernel's arrival counter (re-armed by the forward kernel)
  int heads;            // H (the MH = false kernels do not read it: 1)
  int lhp;              // log2(Hp)  (... 0)
};

__device__ __forceinline__ float make_logit(float dot, int64_t query, int64_t cand,
                                            const SoftmaxArgs &a, float corr_c,
                                            int64_t id_q, int64_t id_c, bool *masked) {
  float v = dot * a.inv_t;
  if (a.corr) v -= corr_c;
  if (a.ids && cand != query && id_c == id_q) v += kMinFloat;
  *masked = false;
  if (a.mask && !a.mask[query * a.nc + cand]) {
    v = kMinFloat;
    *masked = true;
  }
  return v;
}

// Combines the per-split (max, sum) pairs, writes lse/pos and the weighted loss.
// One thread per query row; every block leaves a partial loss in block_part[] and the LAST
// block to finish (ticket counter) adds the partials in block order, so the result does not
// depend on scheduling.  `ticket` must be zero on entry and is reset for the next launch.
static __global__ void __launch_bounds__(256) softmax_finalize_kernel(const SoftmaxArgs a, float *out_loss,
                                                               float *out_lse, float *out_pos,
                                                               double *block_part, uint32_t *ticket) {
  __shared__ double red[256];
  __shared__ bool is_last;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double local = 0.0;
  if (row < a.nq) {
    float mm = -__builtin_inff();
    for (int sp = 0; sp < a.nsplit; ++sp) mm = fmaxf(mm, a.pm[(int64_t)sp * a.nq + row]);
    float ll = 0.0f;
    for (int sp = 0; sp < a.nsplit; ++sp) {
      const float pm = a.pm[(int64_t)sp * a.nq + row];
      if (pm > -__builtin_inff()) ll += a.pl[(int64_t)sp * a.nq + row] * expf(pm - mm);
    }
    const float lse = mm + logf(ll);
    const float pos = a.ppos[row];
    out_lse[row] = lse;
    out_pos[row] = pos;
    const float w = a.w ? a.w[row] : 1.0f;
    // (mm - pos) + log(ll), not lse - pos: for a row whose score_mask is all False mm and pos are both kMinFloat, whose
    // ulp (2.5e29) swallows log(ll) in lse -- the difference first is exact there and the row's loss is log(nc)
    local = (double)w * ((double)(mm - pos) + (double)logf(ll));
  }
  red[threadIdx.x] = local;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&block_part[blockIdx.x], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = (t == gridDim.x - 1);
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double total = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b)
      total += __hip_atomic_load(&block_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *out_loss = (float)total;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static __global__ void __launch_bounds__(256) reduce_partials_kernel(const float *partial, int nsplit,
                                                              int64_t count, float *out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count;
       t += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.0f;
    for (int sp = 0; sp < nsplit; ++sp) acc += partial[(int64_t)sp * count + t];
    out[t] = acc;
  }
}

// How many waves share one block of 32 owned rows (`row_blocks` of them) that streams `tiles`
// 32-row tiles of the other side: the number of splits and their length in rows.
// The planner's target (TFRS_SOFTMAX_WAVES), resolved once per entry-point call -- read per call: tests switch it --
// and handed down to every plan of that call.
static int64_t resolve_target_waves() {
  const char *v = option("TFRS_SOFTMAX_WAVES");
  return (v && *v) ? (int64_t)atoll(v) : (int64_t)2048;  // ~2 waves per SIMD on 256 CUs
}

static void softmax_plan_blocks(int64_t target_waves, int64_t row_blocks, int64_t tiles, int *nsplit,
                                int64_t *split_len) {
  int64_t want = (target_waves + row_blocks - 1) / row_blocks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int64_t per = (tiles + want - 1) / want;
  *split_len = per * 32;
  *nsplit = (int)((tiles + per - 1) / per);
}

static int log2_padded_heads(int heads) {
  int lhp = 0;
  while ((1 << lhp) < heads) ++lhp;
  return lhp;
}

// splits of the forward / dq kernels (waves own query blocks) and of the dc kernel (waves own candidates)
static void plan_queries(int64_t target_waves, int64_t nq, int lhp, int64_t nc, int *nsplit, int64_t *split_len) {
  const int qw = 32 >> lhp;
  softmax_plan_blocks(target_waves, (nq + qw - 1) / qw, (nc + 31) / 32, nsplit, split_len);
}
static void plan_candidates(int64_t target_waves, int64_t nq, int lhp, int64_t nc, int *nsplit, int64_t *split_len) {
  const int qw = 32 >> lhp;
  softmax_plan_blocks(target_waves, (nc + 31) / 32, (nq + qw - 1) / qw, nsplit, split_len);
}

// softmax_finalize_kernel on the [nsplit, nq] partial (max, sum) pairs and the positives of `a`
static void softmax_launch_finalize(const SoftmaxArgs &a, float *out_loss, float *out_lse, float *out_pos,
                                    double *block_part, hipStream_t s) {
  hipLaunchKernelGGL(softmax_finalize_kernel, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, s, a, out_loss,
                     out_lse, out_pos, block_part, a.ticket);
}

// out[t] = sum over the nsplit partial buffers of `count` floats
static void softmax_launch_reduce(const float *partial, int nsplit, int64_t count, float *out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)std::min<int64_t>((count + 255) / 256, 2048)), dim3(256),
                     0, s, partial, nsplit, count, out);
}

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

// f(std::integral_constant<int, DP>) for the padded dim the kernels are instantiated at
template <class F>
static void for_padded_dim(int d, F &&f) {
  switch (softmax_padded_dim(d)) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: f(std::integral_constant<int, 128>{}); break;
  }
}

}  // namespace tfrs
