// topk_merge_heads.hip -- exact top-K of multi-head (max-sim) queries from per-head top-K lists.
//
// BruteForce over queries q[nq, H, d] returns the top-k of  M_bc = max_h (q_bh . c_c)  under (score
// descending, row ascending).  The search itself is the existing 2-D search of the nq * H flat
// (query, head) rows with the SAME k; this kernel merges a query's H lists.
//
// Why the union of the per-head top-k lists contains the top-k of the max: let row c be in the top-k of M_b,
// i.e. fewer than k rows c' precede it under (M descending, row ascending), and let h be a head with
// q_bh . c = M_bc.  A row c' that precedes c in head h's list has q_bh . c' > M_bc, or = M_bc with c' < c;
// since M_bc' >= q_bh . c', that row also precedes c under M.  So fewer than k rows precede c in head h's
// list and c is among that list's first k, with its score there equal to M_bc.  A row can appear in several
// lists with lower scores: the merge keeps its highest.
//
// One workgroup per query holds the H * k_in (score, row) pairs as 64-bit keys in LDS (H * k_in <= 8192:
// 64 KB) and runs two bitonic sorts:
//   1. by (row ascending, score descending): copies of a row become neighbours, the best one first;
//      every later copy is invalidated;
//   2. by (score descending, row ascending) -- the order of every result list of the library (make_key);
//      the first k_out keys are the result.
// Scores pass through as bit patterns (-0.0 is +0.0, as in every key of the library).
#include "common.h"

namespace tfrs {

constexpr int kMergeHeadsMaxPairs = 8192;
constexpr int kMergeHeadsThreads = 256;

// descending bitonic sort of n (a power of two >= 2) keys in LDS by the whole workgroup
__device__ inline void bitonic_sort_desc(uint64_t *keys, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += kMergeHeadsThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const uint64_t x = keys[i], y = keys[p];
        const bool desc = (i & k) == 0;
        if (desc ? (x < y) : (x > y)) {
          keys[i] = y;
          keys[p] = x;
        }
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(kMergeHeadsThreads) merge_heads_kernel(
    const float *scores, const int32_t *rows, int pairs, int n_pow2, int k_out, float *out_scores,
    int32_t *out_rows) {
  extern __shared__ __attribute__((aligned(16))) uint64_t mh_keys[];
  const int64_t query = blockIdx.x;
  const float *s_in = scores + query * pairs;
  const int32_t *r_in = rows + query * pairs;
  // key of sort 1: high word ~row (descending = row ascending), low word the orderable score; 0 = empty
  for (int i = threadIdx.x; i < n_pow2; i += kMergeHeadsThreads) {
    uint64_t key = 0;
    if (i < pairs) {
      const int32_t row = r_in[i];
      if (row >= 0) key = ((uint64_t)(~(uint32_t)row) << 32) | f32_orderable(s_in[i]);
    }
    mh_keys[i] = key;
  }
  __syncthreads();
  bitonic_sort_desc(mh_keys, n_pow2);
  // a key whose row equals its left neighbour's is a lower-or-equal copy: drop it.  Every thread reads
  // its keys and their neighbours before any key is rewritten.
  constexpr int kPer = kMergeHeadsMaxPairs / kMergeHeadsThreads;
  uint64_t mine[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int i = threadIdx.x + e * kMergeHeadsThreads;
    uint64_t key = 0;
    if (i < n_pow2) {
      key = mh_keys[i];
      if (i > 0 && (uint32_t)(mh_keys[i - 1] >> 32) == (uint32_t)(key >> 32)) key = 0;
    }
    mine[e] = (key << 32) | (key >> 32);  // make_key's layout: (orderable score, ~row)
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int i = threadIdx.x + e * kMergeHeadsThreads;
    if (i < n_pow2) mh_keys[i] = mine[e];
  }
  __syncthreads();
  bitonic_sort_desc(mh_keys, n_pow2);
  for (int i = threadIdx.x; i < k_out; i += kMergeHeadsThreads) {
    const uint64_t key = i < n_pow2 ? mh_keys[i] : 0;
    const bool empty = (uint32_t)(key >> 32) == 0u;
    out_scores[query * k_out + i] = empty ? -__builtin_inff() : key_score(key);
    out_rows[query * k_out + i] = empty ? -1 : key_index(key);
  }
}

}  // namespace tfrs

extern "C" int tfrs_topk_merge_heads(const float *scores, const int32_t *rows, int64_t nq, int heads, int k_in,
                                     int k_out, float *out_scores, int32_t *out_rows, void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(nq >= 0 && nq <= 0x7FFFFFFF, "topk_merge_heads: bad nq=%lld", (long long)nq);
  TFRS_CHECK_ARG(heads >= 1 && heads <= 32, "topk_merge_heads: heads=%d outside [1, 32]", heads);
  TFRS_CHECK_ARG(k_in >= 1, "topk_merge_heads: k_in=%d below 1", k_in);
  TFRS_CHECK_ARG((int64_t)heads * k_in <= kMergeHeadsMaxPairs, "topk_merge_heads: heads * k_in = %lld above the %d "
                 "pairs one workgroup holds in LDS", (long long)heads * k_in, kMergeHeadsMaxPairs);
  TFRS_CHECK_ARG(k_in <= TFRS_MAX_K, "topk_merge_heads: k_in=%d outside [1, %d]", k_in, TFRS_MAX_K);
  TFRS_CHECK_ARG(k_out >= 1 && k_out <= k_in, "topk_merge_heads: k_out=%d outside [1, k_in=%d]", k_out, k_in);
  if (nq == 0) return TFRS_OK;
  TFRS_CHECK_ARG(scores && rows && out_scores && out_rows, "topk_merge_heads: NULL pointer");
  const int pairs = heads * k_in;
  int n_pow2 = 2;
  while (n_pow2 < pairs) n_pow2 <<= 1;
  hipLaunchKernelGGL(merge_heads_kernel, dim3((unsigned)nq), dim3(kMergeHeadsThreads), (size_t)n_pow2 * 8,
                     (hipStream_t)stream, scores, rows, pairs, n_pow2, k_out, out_scores, out_rows);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
