// scann.hip -- the search of factorized_top_k.ScaNN (reference layers/factorized_top_k.py:613-796): a partitioned,
// product-quantized approximate top-K.  The index (layers/factorized_top_k.py, ScaNN.index) holds
//   - leaf_offsets[L + 1]: the rows of leaf l are positions leaf_offsets[l] .. leaf_offsets[l + 1] of the leaf-major
//     order, perm[position] is the original row;
//   - codes[n + 128][code_bytes] (128 zero rows of padding at the end): 4-bit codes of the residual x - mu_leaf, block b of dims_per_block
//     dimensions in the low (b even) or high (b odd) nibble of byte b / 2; every leaf is one contiguous byte range;
//   - lut[dp][16] (fp16, dp = d rounded up to 16): the codebook value of dimension i under code c, times 2^lut_exp;
//   - rows[n][d] (f32, leaf-major), only when the layer re-orders.
// One call (one chunk of queries) is: plan (slot offsets, leaf-major work list), AH scan (decode + fp16 MFMA) into a
// [nq, p_max] score buffer, top-R selection (tfrs_topk_update_from_scores), exact re-scoring and the final merge
// (tfrs_topk_merge).  No host synchronisation and no data-dependent host decision: graph capturable.
#include <algorithm>

#include "common.h"

namespace tfrs {

typedef _Float16 sc16h8 __attribute__((ext_vector_type(8)));
typedef float sc32x16 __attribute__((ext_vector_type(16)));

constexpr int kScannRange = 4096;    // rows of one leaf per scan work item
constexpr int kScannTile = 32;       // (query, probe) pairs per scan work item: the MFMA's 32 columns
constexpr int kScannGroupRows = 128; // rows a workgroup decodes per step (4 waves x 32)
constexpr int kScannMaxCodeBytes = 64;

static inline size_t sc_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct ScannWs {
  int32_t *counts, *pstart, *cursor, *wstart, *pairs, *so, *qexp, *sel_c, *map_r;
  _Float16 *q16;
  float *buf, *sel_s, *map_s;
  size_t total;
};

static ScannWs scann_layout(char *base, int64_t nq, int num_leaves, int l_eff, int dp, int64_t p_max, int r) {
  ScannWs w = {};
  size_t off = 0;
  auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += sc_align(bytes); return p; };
  w.counts = (int32_t *)take(sizeof(int32_t) * num_leaves);
  w.pstart = (int32_t *)take(sizeof(int32_t) * (num_leaves + 1));
  w.cursor = (int32_t *)take(sizeof(int32_t) * num_leaves);
  w.wstart = (int32_t *)take(sizeof(int32_t) * (num_leaves + 1));
  w.pairs = (int32_t *)take(sizeof(int32_t) * nq * l_eff);
  w.so = (int32_t *)take(sizeof(int32_t) * nq * (l_eff + 1));
  w.qexp = (int32_t *)take(sizeof(int32_t) * nq);
  w.q16 = (_Float16 *)take(sizeof(_Float16) * nq * dp);
  w.buf = (float *)take(sizeof(float) * nq * p_max);
  w.sel_s = (float *)take(sizeof(float) * nq * r);
  w.sel_c = (int32_t *)take(sizeof(int32_t) * nq * r);
  w.map_s = (float *)take(sizeof(float) * nq * r);
  w.map_r = (int32_t *)take(sizeof(int32_t) * nq * r);
  w.total = off;
  return w;
}

// The per-leaf pair counters, zeroed by a kernel of the same stream (no memset node in a captured graph).
__global__ void __launch_bounds__(256) scann_zero_kernel(int32_t *__restrict__ counts, int num_leaves) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < num_leaves) counts[i] = 0;
}

// Per query: slot offsets so[b][j] = sum of the sizes of probes 0 .. j-1 (so[b][l_eff] = P_b, the probed rows), and
// the number of queries that probe every leaf.
__global__ void __launch_bounds__(256) scann_slots_kernel(const int32_t *__restrict__ probes, int64_t nq, int l_eff,
                                                          const int64_t *__restrict__ leaf_off, int num_leaves,
                                                          int32_t *__restrict__ so, int32_t *__restrict__ counts) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nq) return;
  int32_t acc = 0;
  for (int j = 0; j < l_eff; ++j) {
    const int32_t leaf = probes[b * l_eff + j];
    so[b * (l_eff + 1) + j] = acc;
    if (leaf >= 0 && leaf < num_leaves) {
      acc += (int32_t)(leaf_off[leaf + 1] - leaf_off[leaf]);
      atomicAdd(&counts[leaf], 1);
    }
  }
  so[b * (l_eff + 1) + l_eff] = acc;
}

// One workgroup: exclusive prefix sums over the leaves of the pair counts (pstart, and the scatter cursors) and of the
// scan work items (wstart: ceil(count / 32) query tiles times ceil(size / kScannRange) row ranges per leaf).
__global__ void __launch_bounds__(1024) scann_plan_kernel(const int32_t *__restrict__ counts, int num_leaves,
                                                          const int64_t *__restrict__ leaf_off,
                                                          int32_t *__restrict__ pstart, int32_t *__restrict__ cursor,
                                                          int32_t *__restrict__ wstart) {
  __shared__ int32_t s_p[1024], s_w[1024];
  __shared__ int32_t s_carry[2];
  const int tid = threadIdx.x;
  if (tid == 0) s_carry[0] = s_carry[1] = 0;
  __syncthreads();
  for (int base = 0; base < num_leaves; base += 1024) {
    const int i = base + tid;
    int32_t c = 0, wk = 0;
    if (i < num_leaves) {
      c = counts[i];
      const int64_t size = leaf_off[i + 1] - leaf_off[i];
      const int32_t nr = (int32_t)((size + kScannRange - 1) / kScannRange);
      wk = ((c + kScannTile - 1) / kScannTile) * nr;
    }
    s_p[tid] = c;
    s_w[tid] = wk;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
      const int32_t vp = tid >= s ? s_p[tid - s] : 0;
      const int32_t vw = tid >= s ? s_w[tid - s] : 0;
      __syncthreads();
      s_p[tid] += vp;
      s_w[tid] += vw;
      __syncthreads();
    }
    if (i < num_leaves) {
      const int32_t ps = s_carry[0] + s_p[tid] - c;
      pstart[i] = ps;
      cursor[i] = ps;
      wstart[i] = s_carry[1] + s_w[tid] - wk;
    }
    __syncthreads();
    if (tid == 0) {
      s_carry[0] += s_p[1023];
      s_carry[1] += s_w[1023];
    }
    __syncthreads();
  }
  if (tid == 0) {
    pstart[num_leaves] = s_carry[0];
    wstart[num_leaves] = s_carry[1];
  }
}

// Counting sort of the (query, probe) pairs by leaf.  The order inside a leaf follows the atomics; a pair's scores do
// not depend on it (each output of the scan is one query's column of the MFMA).
__global__ void __launch_bounds__(256) scann_scatter_kernel(const int32_t *__restrict__ probes, int64_t npairs,
                                                            int num_leaves, int32_t *__restrict__ cursor,
                                                            int32_t *__restrict__ pairs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const int32_t leaf = probes[p];
  if (leaf < 0 || leaf >= num_leaves) return;
  const int32_t pos = atomicAdd(&cursor[leaf], 1);
  if (pos >= 0 && pos < npairs) pairs[pos] = (int32_t)p;
}

// One wave per query: the power-of-two scale 2^qexp that puts max|q| into [2^13, 2^14), and the scaled fp16 row
// (zero beyond d).  No finite query overflows fp16 this way; what flushes is below 2^-38 max|q| (include/tfrs_hip.h).
__global__ void __launch_bounds__(256) scann_qprep_kernel(const float *__restrict__ q, int64_t nq, int d, int dp,
                                                          _Float16 *__restrict__ q16, int32_t *__restrict__ qexp) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nq) return;
  float m = 0.f;
  for (int i = lane; i < d; i += 64) m = fmaxf(m, fabsf(q[b * d + i]));
  for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
  int e = 0;
  if (m > 0.f && m <= 3.402823466e38f) {
    int ex;
    frexpf(m, &ex);   // m in [2^(ex-1), 2^ex)
    e = 14 - ex;
  }
  for (int i = lane; i < dp; i += 64)
    q16[b * dp + i] = (_Float16)(i < d ? ldexpf(q[b * d + i], e) : 0.f);
  if (lane == 0) qexp[b] = e;
}

// The tail [P_b, p_max) of every query's score row: -inf, never selected ahead of a probed row.
__global__ void __launch_bounds__(256) scann_fill_kernel(float *__restrict__ buf, int64_t nq, int64_t p_max,
                                                         const int32_t *__restrict__ so, int l_eff) {
  const int64_t total = nq * p_max;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / p_max;
    if (t - b * p_max >= so[b * (l_eff + 1) + l_eff]) buf[t] = -INFINITY;
  }
}

// The AH scan.  Work item = (row range of one leaf, tile of <= 32 pairs that probe it); D[query][row] of one 32-row
// group is KS steps of v_mfma_f32_32x32x16_f16 with the query tile as A (lane: query l & 31, dims 16 kk + 8 h + 0..7)
// and the decoded rows as B (lane: row l & 31, the same dims).  Result lane (row l & 31, h), register r: query
// (r & 3) + 8 (r >> 2) + 4 h.  s~ = acc * 2^-(qexp + lut_exp) + q.mu_leaf lands at column so[b][j] + row_in_leaf.
template <int KS>
__global__ void __launch_bounds__(256) scann_scan_kernel(
    const _Float16 *__restrict__ q16, const int32_t *__restrict__ qexp, const float *__restrict__ leaf_scores,
    int l_eff, int64_t npairs, const int32_t *__restrict__ so, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ pstart, const int32_t *__restrict__ wstart, const int64_t *__restrict__ leaf_off,
    int num_leaves, const uint8_t *__restrict__ codes, int cb, const _Float16 *__restrict__ lut, int lut_exp, int d,
    int dpb, int64_t p_max, float *__restrict__ buf) {
  constexpr int DP = KS * 16;
  __shared__ _Float16 s_lut[DP * 16];
  __shared__ uint16_t s_tab[DP];
  __shared__ __attribute__((aligned(16))) _Float16 s_q[kScannTile * DP];
  __shared__ int32_t s_exp[kScannTile];
  __shared__ float s_mu[kScannTile];
  __shared__ int64_t s_base[kScannTile], s_end[kScannTile];
  __shared__ __attribute__((aligned(16))) uint32_t s_codes[kScannGroupRows * kScannMaxCodeBytes / 4];

  const int w = blockIdx.x;
  if (w >= wstart[num_leaves]) return;   // (the grid is an upper bound on the work items)
  int lo = 0, hi = num_leaves;           // wstart[lo] <= w < wstart[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wstart[mid] <= w) lo = mid;
    else hi = mid;
  }
  const int leaf = lo;
  const int64_t row0 = leaf_off[leaf];
  const int64_t size = leaf_off[leaf + 1] - row0;
  const int nr = (int)((size + kScannRange - 1) / kScannRange);
  const int local = w - wstart[leaf];
  const int tile = local / nr;
  const int rg = local - tile * nr;
  const int p0 = pstart[leaf] + tile * kScannTile;
  const int nt = (int)max<int64_t>(0, min<int64_t>(min(kScannTile, pstart[leaf + 1] - p0), npairs - p0));
  const int64_t r_lo = (int64_t)rg * kScannRange;
  const int64_t nrows = min<int64_t>(size - r_lo, kScannRange);
  const int tid = threadIdx.x;

  for (int i = tid; i < DP * 16; i += 256) s_lut[i] = lut[i];
  for (int i = tid; i < DP; i += 256) s_tab[i] = i < d ? (uint16_t)(i / dpb) : (uint16_t)0xFFFF;
  for (int i = tid; i < kScannTile * DP; i += 256) {
    const int t = i / DP;
    _Float16 v = (_Float16)0.f;
    if (t < nt) {
      const int32_t p = pairs[p0 + t];
      if (p >= 0 && p < npairs) v = q16[(int64_t)(p / l_eff) * DP + (i - t * DP)];
    }
    s_q[i] = v;
  }
  if (tid < kScannTile) {
    int32_t e = 0;
    float mu = 0.f;
    int64_t base = 0, end = 0;
    const int32_t p = tid < nt ? pairs[p0 + tid] : -1;
    if (p >= 0 && p < npairs) {
      const int64_t b = p / l_eff;
      e = qexp[b] + lut_exp;
      mu = leaf_scores[p];
      base = b * p_max + so[b * (l_eff + 1) + (p - b * l_eff)] + r_lo;
      end = (b + 1) * p_max;   // (a p_max below the query's probed rows would be a caller error: never written past)
    }
    s_exp[tid] = e;
    s_mu[tid] = mu;
    s_base[tid] = base;
    s_end[tid] = end;
  }
  __syncthreads();

  const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, h = lane >> 5;
  sc16h8 a[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) a[kk] = *reinterpret_cast<const sc16h8 *>(&s_q[r32 * DP + kk * 16 + 8 * h]);

  const int words = kScannGroupRows * cb / 4;
  const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(s_codes) + (wv * 32 + r32) * cb;
  for (int64_t g0 = 0; g0 < nrows; g0 += kScannGroupRows) {
    // codes of 128 rows (past the range's end: the next leaf's rows or the array's padding, never used)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(codes + (row0 + r_lo + g0) * cb);
    for (int i = tid; i < words; i += 256) s_codes[i] = src[i];
    __syncthreads();
    const int64_t rr = g0 + wv * 32 + r32;
    sc32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      sc16h8 bv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int dim = kk * 16 + 8 * h + e;
        const uint32_t t = s_tab[dim];
        _Float16 v = (_Float16)0.f;
        if (t != 0xFFFFu) v = s_lut[dim * 16 + ((cbytes[t >> 1] >> ((t & 1) * 4)) & 15)];
        bv[e] = v;
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], bv, acc, 0, 0, 0);
    }
    if (rr < nrows) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (qi < nt && s_base[qi] + rr < s_end[qi]) buf[s_base[qi] + rr] = ldexpf(acc[r], -s_exp[qi]) + s_mu[qi];
      }
    }
    __syncthreads();
  }
}

// Selected column -> (score, original row): slot by binary search over the query's slot offsets, leaf-major position,
// perm.  With `rows` the score is the d-ordered f32 fma chain of BruteForce / oracle.topk.scores, else s~.  Columns
// outside [0, P_b) (the -inf tail) become (-inf, INT32_MAX): last under (score desc, row asc).
__global__ void __launch_bounds__(256) scann_map_kernel(const float *__restrict__ sel_s,
                                                        const int32_t *__restrict__ sel_c, int64_t nq, int r,
                                                        const int32_t *__restrict__ so, int l_eff,
                                                        const int32_t *__restrict__ probes,
                                                        const int64_t *__restrict__ leaf_off,
                                                        const int32_t *__restrict__ perm, const float *__restrict__ rows,
                                                        const float *__restrict__ queries, int d,
                                                        float *__restrict__ map_s, int32_t *__restrict__ map_r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * r) return;
  const int64_t b = i / r;
  const int32_t col = sel_c[i];
  const int32_t *sob = so + b * (l_eff + 1);
  float s = -INFINITY;
  int32_t row = 0x7FFFFFFF;
  if (col >= 0 && col < sob[l_eff]) {
    int lo = 0, hi = l_eff;   // sob[lo] <= col < sob[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sob[mid] <= col) lo = mid;
      else hi = mid;
    }
    const int64_t pos = leaf_off[probes[b * l_eff + lo]] + (col - sob[lo]);
    row = perm[pos];
    if (rows) {
      const float *x = rows + pos * d;
      const float *qb = queries + b * d;
      float acc = 0.f;
      for (int c = 0; c < d; ++c) acc = fmaf(qb[c], x[c], acc);
      s = acc;
    } else {
      s = sel_s[i];
    }
  }
  map_s[i] = s;
  map_r[i] = row;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" size_t tfrs_scann_search_workspace_bytes(int64_t nq, int num_leaves, int l_eff, int d, int64_t p_max,
                                                    int r) {
  if (nq < 1 || num_leaves < 1 || l_eff < 1 || d < 1 || p_max < 1 || r < 1) return 0;
  const int dp = (d + 15) / 16 * 16;
  return scann_layout(nullptr, nq, num_leaves, l_eff, dp, p_max, (int)std::min<int64_t>(r, p_max)).total;
}

extern "C" int tfrs_scann_search(const float *queries, int64_t nq, int d, const int32_t *probes,
                                 const float *leaf_scores, int l_eff, const int64_t *leaf_offsets, int num_leaves,
                                 int64_t max_leaf_rows, const uint8_t *codes, int code_bytes, const void *lut,
                                 int dims_per_block, int lut_exp, const int32_t *perm, const float *rows,
                                 int64_t p_max, int r, int k, float *out_scores, int32_t *out_rows, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  TFRS_CHECK_ARG(nq >= 0 && d >= 1 && d <= TFRS_MAX_DIM, "scann_search: dim=%d outside [1, %d]", d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(num_leaves >= 1 && l_eff >= 1 && l_eff <= num_leaves,
                 "scann_search: l_eff=%d must be in [1, num_leaves=%d]", l_eff, num_leaves);
  TFRS_CHECK_ARG(dims_per_block >= 1 && dims_per_block <= d, "scann_search: dims_per_block=%d", dims_per_block);
  const int nblocks = (d + dims_per_block - 1) / dims_per_block;
  TFRS_CHECK_ARG(code_bytes % 4 == 0 && code_bytes >= (nblocks + 1) / 2 && code_bytes <= kScannMaxCodeBytes,
                 "scann_search: code_bytes=%d (multiple of 4, >= %d, <= %d)", code_bytes, (nblocks + 1) / 2,
                 kScannMaxCodeBytes);
  TFRS_CHECK_ARG(k >= 1 && k <= TFRS_MAX_K && r >= k && r <= TFRS_MAX_K,
                 "scann_search: need 1 <= k=%d <= r=%d <= %d", k, r, TFRS_MAX_K);
  TFRS_CHECK_ARG(p_max >= k && p_max <= 0x7FFFFFFFll, "scann_search: p_max=%lld must be in [k, 2^31)",
                 (long long)p_max);
  TFRS_CHECK_ARG(max_leaf_rows >= 1, "scann_search: max_leaf_rows=%lld", (long long)max_leaf_rows);
  TFRS_CHECK_ARG(nq * (int64_t)l_eff <= 0x7FFFFFFFll, "scann_search: nq * l_eff exceeds int32");
  if (nq == 0) return TFRS_OK;
  TFRS_CHECK_ARG(queries && probes && leaf_scores && leaf_offsets && codes && lut && perm && out_scores && out_rows &&
                     workspace, "scann_search: NULL pointer");
  const int ks = (d + 15) / 16;
  const int dp = ks * 16;
  const int re = (int)std::min<int64_t>(r, p_max);
  ScannWs w = scann_layout((char *)workspace, nq, num_leaves, l_eff, dp, p_max, re);
  if (w.total > workspace_bytes) {
    set_error("scann_search: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
    return TFRS_ENOMEM;
  }
  // upper bound on the work items: sum over probed leaves of ceil(c_l / 32) <= nq l_eff / 32 + min(L, nq l_eff)
  // query tiles, each times the row ranges of the largest leaf
  const int64_t npairs = nq * l_eff;
  const int64_t tiles = (npairs + kScannTile - 1) / kScannTile + std::min<int64_t>(num_leaves, npairs);
  const int64_t bound = tiles * ((max_leaf_rows + kScannRange - 1) / kScannRange);
  TFRS_CHECK_ARG(bound <= 0x7FFFFFFFll, "scann_search: %lld scan work items exceed the grid", (long long)bound);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(scann_zero_kernel, dim3((unsigned)((num_leaves + 255) / 256)), dim3(256), 0, st, w.counts,
                     num_leaves);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scann_slots_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, probes, nq, l_eff,
                     leaf_offsets, num_leaves, w.so, w.counts);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scann_plan_kernel, dim3(1), dim3(1024), 0, st, w.counts, num_leaves, leaf_offsets, w.pstart,
                     w.cursor, w.wstart);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scann_scatter_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st, probes, npairs,
                     num_leaves, w.cursor, w.pairs);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(scann_qprep_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, queries, nq, d, dp, w.q16,
                     w.qexp);
  TFRS_LAUNCH_CHECK();
  const int64_t cells = nq * p_max;
  hipLaunchKernelGGL(scann_fill_kernel, dim3((unsigned)std::min<int64_t>((cells + 255) / 256, 65536)), dim3(256), 0,
                     st, w.buf, nq, p_max, w.so, l_eff);
  TFRS_LAUNCH_CHECK();
  const _Float16 *lut16 = reinterpret_cast<const _Float16 *>(lut);
#define TFRS_SCANN_SCAN(KS)                                                                                          \
  hipLaunchKernelGGL(scann_scan_kernel<KS>, dim3((unsigned)bound), dim3(256), 0, st, w.q16, w.qexp, leaf_scores,   \
                     l_eff, npairs, w.so, w.pairs, w.pstart, w.wstart, leaf_offsets, num_leaves, codes, code_bytes, lut16,  \
                     lut_exp, d, dims_per_block, p_max, w.buf)
  switch (ks) {
    case 1: TFRS_SCANN_SCAN(1); break;
    case 2: TFRS_SCANN_SCAN(2); break;
    case 3: TFRS_SCANN_SCAN(3); break;
    case 4: TFRS_SCANN_SCAN(4); break;
    case 5: TFRS_SCANN_SCAN(5); break;
    case 6: TFRS_SCANN_SCAN(6); break;
    case 7: TFRS_SCANN_SCAN(7); break;
    default: TFRS_SCANN_SCAN(8); break;
  }
#undef TFRS_SCANN_SCAN
  TFRS_LAUNCH_CHECK();
  int rc = tfrs_topk_update_from_scores(w.buf, nq, p_max, p_max, 0, re, w.sel_s, w.sel_c, 0, nullptr, stream);
  if (rc != TFRS_OK) return rc;
  hipLaunchKernelGGL(scann_map_kernel, dim3((unsigned)((nq * re + 255) / 256)), dim3(256), 0, st, w.sel_s, w.sel_c,
                     nq, re, w.so, l_eff, probes, leaf_offsets, perm, rows, queries, d, w.map_s, w.map_r);
  TFRS_LAUNCH_CHECK();
  return tfrs_topk_merge(w.map_s, w.map_r, 1, nq, re, k, out_scores, out_rows, nullptr, 0, stream);
}
