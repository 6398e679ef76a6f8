// embedding.hip -- embedding row gather, segment (combiner) reduce forward and backward, the deterministic scatter-add
// backward over PRESORTED ids (tfrs_embedding_scatter_add_bwd) and the one-launch copy of a batch's input tensors.
// Every sparse optimizer update -- the radix sort, the scatter-add / Adagrad of unsorted ids, the row scan, Clippy, the
// rule kernels and row-wise Adagrad -- lives in sparse_update.hip.
//
// Replaces tf.gather behind tf.keras.layers.Embedding (README.md:62-66,77-78), the
// combiner lookup of the TPUEmbedding CPU branch
// (layers/embedding/tpu_embedding_layer.py:913-919) and the IndexedSlices gradient +
// optimizer.apply_gradients of tfrs.Model.train_step (models/base.py:77-78).
//
// All three are HBM-bound byte movers.  Layout rule: a table row is read/written as
// 16-byte pieces by D/4 consecutive lanes, so a wave touches 64/(D/4) whole rows per
// instruction (full 128..512-byte lines), with several independent row loads in flight
// per lane to cover the ~2 us random-HBM latency.  Algorithmic bytes per gathered row:
// D*4 read + D*4 written + the id.
#include <type_traits>

#include "common.h"
#include "row_access.h"
#include "table_rules.h"

namespace tfrs {

// ---- dense gather ---------------------------------------------------------------------
// VEC = 4: d % 4 == 0 (16-byte pieces); VEC = 1: any d.
template <typename IdT, int VEC, int UNROLL = 4, bool NT = false>
__global__ void __launch_bounds__(256) gather_kernel(const float *__restrict__ table,
                                                     int64_t vocab, int d,
                                                     const void *__restrict__ ids, int64_t n,
                                                     float *__restrict__ out,
                                                     int32_t *err_flag) {
  const int per_row = d / VEC;
  const int64_t total = n * per_row;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; t + (UNROLL - 1) * stride < total; t += UNROLL * stride) {
    int64_t src[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t e = t + u * stride;
      const int64_t row = e / per_row;
      const int c = (int)(e - row * per_row);
      const int64_t id = load_id<IdT>(ids, row);
      ok[u] = (id >= 0 && id < vocab);
      src[u] = (ok[u] ? id : 0) * per_row + c;
    }
    if (VEC == 4) {
      float4 v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const float4 *sp = reinterpret_cast<const float4 *>(table) + src[u];
        if (NT) {
          typedef float f4 __attribute__((ext_vector_type(4)));
          const f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(sp));
          v[u] = make_float4(x[0], x[1], x[2], x[3]);
        } else {
          v[u] = *sp;
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (!ok[u]) {
          v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (err_flag) *err_flag = 1;
        }
        float4 *dp = reinterpret_cast<float4 *>(out) + (t + u * stride);
        if (NT) {
          typedef float f4 __attribute__((ext_vector_type(4)));
          f4 x = {v[u].x, v[u].y, v[u].z, v[u].w};
          __builtin_nontemporal_store(x, reinterpret_cast<f4 *>(dp));
        } else {
          *dp = v[u];
        }
      }
    } else {
      float v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = table[src[u]];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (!ok[u]) {
          v[u] = 0.f;
          if (err_flag) *err_flag = 1;
        }
        out[t + u * stride] = v[u];
      }
    }
  }
  for (; t < total; t += stride) {
    const int64_t row = t / per_row;
    const int c = (int)(t - row * per_row);
    const int64_t id = load_id<IdT>(ids, row);
    const bool ok = (id >= 0 && id < vocab);
    if (!ok && err_flag) *err_flag = 1;
    if (VEC == 4) {
      float4 v = ok ? reinterpret_cast<const float4 *>(table)[id * per_row + c]
                    : make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4 *>(out)[t] = v;
    } else {
      out[t] = ok ? table[id * per_row + c] : 0.f;
    }
  }
}

// ---- segment reduce (sum / mean / sqrtn combiner) -------------------------------------
// One group of `per_row` lanes per output row; the group walks the row's id segment in
// order (so the float32 sum order is the id order, like the oracle).
template <typename IdT, int VEC>
__global__ void __launch_bounds__(256) segment_reduce_kernel(
    const float *__restrict__ table, int64_t vocab, int d, const void *__restrict__ ids,
    const void *__restrict__ row_splits, const float *__restrict__ weights, int64_t nrows,
    int combiner, float *__restrict__ out, int32_t *err_flag) {
  const int per_row = d / VEC;
  const int64_t total = nrows * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / per_row;
    const int c = (int)(t - row * per_row);
    const int64_t lo = load_id<IdT>(row_splits, row), hi = load_id<IdT>(row_splits, row + 1);
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    float wsum = 0.f, wsq = 0.f;
    // Eight entries per round: their ids and weights are fetched as one batch of independent loads,
    // then their row pieces as a second batch, then they are added IN ORDER (the float32 sum order
    // stays the id order).  The entry-at-a-time loop it replaces paid two dependent memory round
    // trips per entry (0.61 of HBM at bags of 8).
    // Every load of a round is UNCONDITIONAL (entries past the segment's end re-read its last entry, bad ids
    // read row 0; both are discarded by selects afterwards): a load inside a branch -- `in ? ids[p] : -1`,
    // `if (ok) x = row` -- makes the number of loads in flight unknown to the compiler, which then waits for
    // every load before issuing the next (vmcnt(0)), and the round is eight serial round trips again.
    constexpr int kU = 8;
    auto rounds = [&](auto has_w) __attribute__((always_inline)) {
      for (int64_t p0 = lo; p0 < hi; p0 += kU) {
        int64_t idv[kU];
        float wv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int64_t p = p0 + u < hi ? p0 + u : hi - 1;
          idv[u] = load_id<IdT>(ids, p);
          wv[u] = decltype(has_w)::value ? weights[p] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          if (!(p0 + u < hi)) {
            idv[u] = -1;
            wv[u] = 0.0f;
          }
        }
        float ev[kU][VEC];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const bool ok = idv[u] >= 0 && idv[u] < vocab;
          const int64_t src = (ok ? idv[u] : 0) * per_row + c;
          if (VEC == 4) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            const f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(table) + src);
#pragma unroll
            for (int v = 0; v < VEC; ++v) ev[u][v] = x[v];
          } else {
            ev[u][0] = table[src];
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          if (p0 + u < hi) {
            wsum += wv[u];
            wsq = __builtin_fmaf(wv[u], wv[u], wsq);
            if (idv[u] < 0 || idv[u] >= vocab) {
              if (err_flag) *err_flag = 1;
            } else {
#pragma unroll
              for (int v = 0; v < VEC; ++v) acc[v] += wv[u] * ev[u][v];
            }
          }
        }
      }
    };
    if (weights) rounds(std::true_type{}); else rounds(std::false_type{});
    float scale = 1.0f;
    if (hi > lo) {
      if (combiner == 1) scale = 1.0f / wsum;
      if (combiner == 2) scale = 1.0f / sqrtf(wsq);
    }
    if (VEC == 4) {
      float4 o;
      if (combiner == 0) {
        o = make_float4(acc[0], acc[1 % VEC], acc[2 % VEC], acc[3 % VEC]);
      } else {  // divide (not multiply by the reciprocal) to match acc / sum(w)
        const float den = (hi > lo) ? (combiner == 1 ? wsum : sqrtf(wsq)) : 1.0f;
        o = make_float4(acc[0] / den, acc[1 % VEC] / den, acc[2 % VEC] / den, acc[3 % VEC] / den);
      }
      reinterpret_cast<float4 *>(out)[t] = o;
    } else {
      const float den = (hi > lo && combiner != 0) ? (combiner == 1 ? wsum : sqrtf(wsq)) : 1.0f;
      out[t] = acc[0] / den;
    }
    (void)scale;
  }
}

// ---- segment (combiner) reduce backward ---------------------------------------------------
// d out[b] / d e_p = w_p / den_b for every entry p of segment b (den as in the forward), so the
// gradient rows of the nnz looked-up entries are grad_rows[p] = (grad_out[b] / den_b) * w_p:
// the IndexedSlices form (ids, grad_rows) the scatter-add / sparse Adagrad kernels consume.
// Same lane mapping as the forward (D/4 lanes per segment): grad_out read once per segment,
// nnz*D*4 bytes written.
template <typename IdT, int VEC>
__global__ void __launch_bounds__(256) segment_reduce_bwd_kernel(
    const float *__restrict__ grad_out, int d, const void *__restrict__ row_splits,
    const float *__restrict__ weights, int64_t nrows, int combiner,
    float *__restrict__ grad_rows) {
  const int per_row = d / VEC;
  const int64_t total = nrows * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / per_row;
    const int c = (int)(t - row * per_row);
    const int64_t lo = load_id<IdT>(row_splits, row), hi = load_id<IdT>(row_splits, row + 1);
    if (hi <= lo) continue;
    float den = 1.0f;
    if (combiner != 0) {
      float wsum = 0.f, wsq = 0.f;
      for (int64_t p = lo; p < hi; ++p) {
        const float w = weights ? weights[p] : 1.0f;
        wsum += w;
        wsq = __builtin_fmaf(w, w, wsq);
      }
      den = combiner == 1 ? wsum : sqrtf(wsq);
    }
    float g[VEC];
    if (VEC == 4) {
      const float4 gv = reinterpret_cast<const float4 *>(grad_out)[t];
      g[0] = gv.x / den;
      g[1 % VEC] = gv.y / den;
      g[2 % VEC] = gv.z / den;
      g[3 % VEC] = gv.w / den;
    } else {
      g[0] = grad_out[t] / den;
    }
    for (int64_t p = lo; p < hi; ++p) {
      const float w = weights ? weights[p] : 1.0f;
      if (VEC == 4) {
        reinterpret_cast<float4 *>(grad_rows)[p * per_row + c] =
            make_float4(g[0] * w, g[1 % VEC] * w, g[2 % VEC] * w, g[3 % VEC] * w);
      } else {
        grad_rows[p * per_row + c] = g[0] * w;
      }
    }
  }
}

// ---- scatter-add backward (+ fused Adagrad) --------------------------------------------
// Input: ids sorted ascending (stable) with perm[i] = original position.  A lane group
// owns every position that starts a run of equal ids and sums the run's gradient rows in
// occurrence order: no atomics, bit-reproducible, duplicates summed BEFORE the optimizer
// update as Keras does for IndexedSlices.
template <int VEC>
__global__ void __launch_bounds__(256) scatter_add_kernel(
    const float *__restrict__ grad_out, const int64_t *__restrict__ sorted_ids,
    const int64_t *__restrict__ perm, int64_t n, int d, float *__restrict__ dst,
    float *__restrict__ accum, float lr, float eps, int adagrad) {
  const int per_row = d / VEC;
  const int64_t total = n * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per_row;
    const int c = (int)(t - i * per_row);
    const int64_t id = sorted_ids[i];
    if (id < 0) continue;                            // padding slot of a sequence feature
    if (i > 0 && sorted_ids[i - 1] == id) continue;  // not the start of a run
    float g[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] = 0.f;
    for (int64_t p = i; p < n && sorted_ids[p] == id; ++p) {
      const int64_t src = perm[p];
      if (VEC == 4) {
        const float4 e = reinterpret_cast<const float4 *>(grad_out)[src * per_row + c];
        g[0] += e.x;
        g[1 % VEC] += e.y;
        g[2 % VEC] += e.z;
        g[3 % VEC] += e.w;
      } else {
        g[0] += grad_out[src * per_row + c];
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int64_t o = (id * per_row + c) * VEC + v;
      if (adagrad) {
        const float a = accum[o] + g[v] * g[v];
        accum[o] = a;
        dst[o] = dst[o] - lr * g[v] / adagrad_denom(a, eps, adagrad);
      } else {
        dst[o] = g[v];
      }
    }
  }
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_embedding_gather_fwd(const float *table, int64_t vocab, int d,
                                         const void *ids, int ids_are_i64, int64_t n,
                                         float *out, int32_t *err_flag, void *stream) {
  TFRS_CHECK_ARG(vocab >= 1 && d >= 1 && n >= 0, "embedding_gather: bad shape");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG(table && ids && out, "embedding_gather: NULL pointer");
  const bool vec = (d % 4 == 0) && (((uintptr_t)table | (uintptr_t)out) % 16 == 0);
  const int64_t total = n * (vec ? d / 4 : d);
  // Rows are read once and the output is written once: non-temporal loads/stores and a
  // grid of up to 64 workgroups per CU measured 6.4 TB/s (read + written) on 26M x 128
  // against 5.4 TB/s for cached accesses with 8 workgroups per CU (tools/exp_gather.py).
  const dim3 grid(grid_for((total + 3) / 4, 256 * 64)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (ids_are_i64) {
    if (vec)
      hipLaunchKernelGGL((gather_kernel<int64_t, 4, 4, true>), grid, block, 0, s, table, vocab, d, ids, n, out, err_flag);
    else
      hipLaunchKernelGGL((gather_kernel<int64_t, 1>), grid, block, 0, s, table, vocab, d, ids, n, out, err_flag);
  } else {
    if (vec)
      hipLaunchKernelGGL((gather_kernel<int32_t, 4, 4, true>), grid, block, 0, s, table, vocab, d, ids, n, out, err_flag);
    else
      hipLaunchKernelGGL((gather_kernel<int32_t, 1>), grid, block, 0, s, table, vocab, d, ids, n, out, err_flag);
  }
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_embedding_segment_reduce_fwd(const float *table, int64_t vocab, int d,
                                                 const void *ids, const void *row_splits,
                                                 int ids_are_i64, const float *weights,
                                                 int64_t nrows, int combiner, float *out,
                                                 int32_t *err_flag, void *stream) {
  TFRS_CHECK_ARG(vocab >= 1 && d >= 1 && nrows >= 0, "embedding_segment_reduce: bad shape");
  TFRS_CHECK_ARG(combiner >= 0 && combiner <= 2,
                 "embedding_segment_reduce: combiner must be 0 (sum), 1 (mean) or 2 (sqrtn)");
  if (nrows == 0) return TFRS_OK;
  TFRS_CHECK_ARG(table && row_splits && out, "embedding_segment_reduce: NULL pointer");
  const bool vec = (d % 4 == 0) && (((uintptr_t)table | (uintptr_t)out) % 16 == 0);
  const int64_t total = nrows * (vec ? d / 4 : d);
  const dim3 grid(grid_for(total, 256 * 64)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (ids_are_i64) {
    if (vec)
      hipLaunchKernelGGL((segment_reduce_kernel<int64_t, 4>), grid, block, 0, s, table, vocab, d, ids, row_splits, weights, nrows, combiner, out, err_flag);
    else
      hipLaunchKernelGGL((segment_reduce_kernel<int64_t, 1>), grid, block, 0, s, table, vocab, d, ids, row_splits, weights, nrows, combiner, out, err_flag);
  } else {
    if (vec)
      hipLaunchKernelGGL((segment_reduce_kernel<int32_t, 4>), grid, block, 0, s, table, vocab, d, ids, row_splits, weights, nrows, combiner, out, err_flag);
    else
      hipLaunchKernelGGL((segment_reduce_kernel<int32_t, 1>), grid, block, 0, s, table, vocab, d, ids, row_splits, weights, nrows, combiner, out, err_flag);
  }
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_embedding_segment_reduce_bwd(const float *grad_out, int d,
                                                 const void *row_splits, int splits_are_i64,
                                                 const float *weights, int64_t nrows,
                                                 int combiner, float *grad_rows, void *stream) {
  TFRS_CHECK_ARG(d >= 1 && nrows >= 0, "embedding_segment_reduce_bwd: bad shape");
  TFRS_CHECK_ARG(combiner >= 0 && combiner <= 2,
                 "embedding_segment_reduce_bwd: combiner must be 0 (sum), 1 (mean) or 2 (sqrtn)");
  if (nrows == 0) return TFRS_OK;
  TFRS_CHECK_ARG(grad_out && row_splits && grad_rows, "embedding_segment_reduce_bwd: NULL pointer");
  const bool vec = (d % 4 == 0) && (((uintptr_t)grad_out | (uintptr_t)grad_rows) % 16 == 0);
  const int64_t total = nrows * (vec ? d / 4 : d);
  const dim3 grid(grid_for(total, 256 * 64)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (splits_are_i64) {
    if (vec)
      hipLaunchKernelGGL((segment_reduce_bwd_kernel<int64_t, 4>), grid, block, 0, s, grad_out, d, row_splits, weights, nrows, combiner, grad_rows);
    else
      hipLaunchKernelGGL((segment_reduce_bwd_kernel<int64_t, 1>), grid, block, 0, s, grad_out, d, row_splits, weights, nrows, combiner, grad_rows);
  } else {
    if (vec)
      hipLaunchKernelGGL((segment_reduce_bwd_kernel<int32_t, 4>), grid, block, 0, s, grad_out, d, row_splits, weights, nrows, combiner, grad_rows);
    else
      hipLaunchKernelGGL((segment_reduce_bwd_kernel<int32_t, 1>), grid, block, 0, s, grad_out, d, row_splits, weights, nrows, combiner, grad_rows);
  }
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_embedding_scatter_add_bwd(const float *grad_out, const int64_t *sorted_ids,
                                              const int64_t *perm, int64_t n, int d,
                                              float *grad_table_or_table, float *accum,
                                              float lr, float eps, int adagrad, void *stream) {
  TFRS_CHECK_ARG(n >= 0 && d >= 1, "embedding_scatter_add: bad shape");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG(grad_out && sorted_ids && perm && grad_table_or_table,
                 "embedding_scatter_add: NULL pointer");
  TFRS_CHECK_ARG(!adagrad || accum, "embedding_scatter_add: Adagrad needs an accumulator");
  const bool vec = (d % 4 == 0) && (((uintptr_t)grad_out) % 16 == 0);
  const int64_t total = n * (vec ? d / 4 : d);
  const dim3 grid(grid_for(total)), block(256);
  if (vec)
    hipLaunchKernelGGL((scatter_add_kernel<4>), grid, block, 0, (hipStream_t)stream, grad_out, sorted_ids, perm, n, d, grad_table_or_table, accum, lr, eps, adagrad);
  else
    hipLaunchKernelGGL((scatter_add_kernel<1>), grid, block, 0, (hipStream_t)stream, grad_out, sorted_ids, perm, n, d, grad_table_or_table, accum, lr, eps, adagrad);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- a batch's input tensors -> the static buffers of a captured step, ONE launch ----------------------------------
// `Model.fit` replays a captured train step on static input buffers; the batch (two id vectors of 32 KB at the quickstart
// shapes) was copied in by torch._foreach_copy_: 6.0-6.4 us of a 113 us step for 64 KB.  Buffer t owns blocks
// [first_block[t], first_block[t + 1]) of 256 threads x 4 x 16 bytes.
namespace tfrs {
struct CopyBuffers {
  int n;
  int first_block[17];
  char *dst[16];
  const char *src[16];
  int64_t bytes[16];
};
constexpr int kCopyPerBlock = 256 * 64;
__global__ void __launch_bounds__(256) copy_multi_kernel(const CopyBuffers t) {
  int k = 0;
  while (k + 1 < t.n && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
  char *__restrict__ dst = t.dst[k];
  const char *__restrict__ src = t.src[k];
  const int64_t n = t.bytes[k];
  const int64_t base = (int64_t)((int)blockIdx.x - t.first_block[k]) * kCopyPerBlock;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0 && n >= 16;
  if (vec) {
    // unconditional (clamped) loads first, then the stores: one memory round trip per block
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = base + (int64_t)(u * 256 + threadIdx.x) * 16;
      v[u] = *reinterpret_cast<const uint4 *>(src + (o + 16 <= n ? o : 0));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = base + (int64_t)(u * 256 + threadIdx.x) * 16;
      if (o + 16 <= n) *reinterpret_cast<uint4 *>(dst + o) = v[u];
    }
    // the last n % 16 bytes of the buffer: the block that owns them
    const int64_t tail = n & ~(int64_t)15;
    if (tail >= base && tail < base + kCopyPerBlock && (int64_t)threadIdx.x < n - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
    return;
  }
  for (int64_t o = base + threadIdx.x; o < n && o < base + kCopyPerBlock; o += 256) dst[o] = src[o];
}
}  // namespace tfrs

extern "C" int tfrs_copy_multi(int nbuffers, void *const *dst_h, const void *const *src_h, const int64_t *bytes_h,
                               void *stream) {
  TFRS_CHECK_ARG(nbuffers >= 1 && nbuffers <= 16, "copy_multi: 1..16 buffers");
  TFRS_CHECK_ARG(dst_h && src_h && bytes_h, "copy_multi: NULL argument array");
  tfrs::CopyBuffers t = {};
  t.n = nbuffers;
  int64_t blocks = 0;
  for (int i = 0; i < nbuffers; ++i) {
    TFRS_CHECK_ARG(bytes_h[i] >= 0 && (bytes_h[i] == 0 || (dst_h[i] && src_h[i])), "copy_multi: bad buffer %d", i);
    t.first_block[i] = (int)blocks;
    blocks += (bytes_h[i] + tfrs::kCopyPerBlock - 1) / tfrs::kCopyPerBlock;
    TFRS_CHECK_ARG(blocks < (1ll << 31), "copy_multi: too many bytes for one launch");
    t.dst[i] = static_cast<char *>(dst_h[i]); t.src[i] = static_cast<const char *>(src_h[i]); t.bytes[i] = bytes_h[i];
  }
  t.first_block[nbuffers] = (int)blocks;
  if (blocks == 0) return TFRS_OK;
  hipLaunchKernelGGL(tfrs::copy_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
