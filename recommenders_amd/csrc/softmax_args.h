// softmax_args.h -- what the in-batch softmax kernels of softmax.hip (2-D queries) and
// softmax_mh.hip (multi-head queries) share: the argument block, the logit function and the
// host entry points of the small deterministic reduce kernels that live in softmax.hip.
#pragma once

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

// softmax.hip.  How many waves share one block of 32 owned rows (`row_blocks` of them) that
// streams `tiles` 32-row tiles of the other side: the number of splits and their length in rows.
void softmax_plan_blocks(int64_t row_blocks, int64_t tiles, int *nsplit, int64_t *split_len);
// softmax_finalize_kernel on the [nsplit, nq] partial (max, sum) pairs and the positives of `a`
void softmax_launch_finalize(const SoftmaxArgs &a, float *out_loss, float *out_lse, float *out_pos,
                             double *block_part, hipStream_t s);
// out[t] = sum over the nsplit partial buffers of `count` floats
void softmax_launch_reduce(const float *partial, int nsplit, int64_t count, float *out, hipStream_t s);

}  // namespace tfrs
