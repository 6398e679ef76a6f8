// sparse_update.hip -- every optimizer update on the looked-up rows of an embedding table, from UNSORTED ids:
// scatter-add / fused Adagrad (tfrs_embedding_scatter_add_unsorted*, *_rowscan*), ClippyAdagrad (tfrs_clippy_sparse*),
// the rules of table_rules.h (tfrs_table_update_sparse: SGD, Adam, Ftrl) and row-wise Adagrad
// (tfrs_rowwise_adagrad_sparse).  Two routes, both deterministic and without atomics, duplicates summed in occurrence
// order BEFORE the update as Keras does for IndexedSlices: the own radix sort below + one lane (group) per run of equal
// ids, or for small tables the row scan (one wave per table row, no sort).  The run sum and the scan are written once
// in sparse_update.h; a kernel here is its own first round of loads, one of the two sums, and its arithmetic.  The
// dense halves of the same optimizers are in table_update.hip, the lookups in embedding.hip.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "clippy.h"
#include "sparse_update.h"
#include "table_rules.h"

// ------------------------------------------------------------------------------------------------
// Own stable LSD radix sort of (id, position) pairs for the large-vocabulary scatter-add
// (replaces torch.sort / rocPRIM on the backward path of models/base.py:77-78).
//   keys   uint32 ids; ids outside [0, vocab) -- the padding slots of sequence features and
//          anything invalid -- become 0xFFFFFFFF: they sort last and the scatter skips them, so
//          an out-of-range id can never write outside the table (the gather reads it as zeros)
//   passes 8, 9 or 10 bits each (more than 8 when that saves a pass: 26 M rows need 26 bits = 3 x 9 instead
//          of 4 x 8, 100 M rows 28 = 3 x 10; a pass is four launch-latency-bound kernels, 47 us at 1.7 M keys); every pass = tile histograms ->
//          exclusive scan (digit-major) -> stable scatter
//   tile   4096 keys per 256-thread workgroup; wave w owns keys [1024 w, 1024 w + 1024) of the
//          tile and walks them 64 at a time IN ORDER: equal digits of one step are ranked with
//          8 .. 10 ballots (lanes with the same digit form a mask; rank = popcount below the lane), the
//          wave's running per-digit offsets live in LDS.  Stable by construction.
// Integer work, HBM-trivial (16 bytes per key and pass); launch-latency bound below ~1M keys.
// ------------------------------------------------------------------------------------------------
namespace tfrs {
constexpr int kSortTile = 4096;

template <int BITS>
__device__ __forceinline__ uint64_t same_digit_mask(uint32_t digit) {
  uint64_t m = ~0ull;
#pragma unroll
  for (int bit = 0; bit < BITS; ++bit) {
    const uint64_t bal = __ballot((digit >> bit) & 1u);
    m &= ((digit >> bit) & 1u) ? bal : ~bal;
  }
  return m;
}

// keys_out[i] = id or 0xFFFFFFFF, vals_out[i] = i  (pass 0 reads these)
__global__ void __launch_bounds__(256) sort_init_kernel(const void *__restrict__ ids, int i64, int64_t n,
                                                        int64_t vocab, uint32_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t id = i64 ? static_cast<const int64_t *>(ids)[i] : (int64_t)static_cast<const int32_t *>(ids)[i];
  keys[i] = (id >= 0 && id < vocab) ? (uint32_t)id : 0xFFFFFFFFu;
  vals[i] = (uint32_t)i;
}

// hist[tile][wave][digit]
template <int BITS>
__global__ void __launch_bounds__(256) sort_hist_kernel(const uint32_t *__restrict__ keys, int64_t n,
                                                        int shift, uint32_t *__restrict__ hist) {
  constexpr int NB = 1 << BITS;
  __shared__ uint32_t h[4][NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 4 * NB; e += 256) (&h[0][0])[e] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile + wave * 1024;
  uint32_t kv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {   // unconditional, at a clamped index: 16 loads in flight (guarded, each was awaited)
    const int64_t i = base + r * 64 + lane;
    kv[r] = keys[i < n ? i : n - 1];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (base + r * 64 + lane < n) atomicAdd(&h[wave][(kv[r] >> shift) & (uint32_t)(NB - 1)], 1u);
  __syncthreads();
  for (int e = tid; e < 4 * NB; e += 256) hist[(int64_t)blockIdx.x * (4 * NB) + e] = (&h[0][0])[e];
}

// Exclusive scan of the segment histograms in digit-major order, two levels (thread = digit):
//   scan1: workgroup c scans its chunk of 64 segments -> offs[segment][digit] (chunk-local) and
//          chunk_tot[c][digit];
//   scan2: one workgroup turns chunk_tot into chunk_base[c][digit] = keys with a smaller digit
//          anywhere + keys with the same digit in earlier chunks.
// The scatter kernel adds the two.
constexpr int kScanChunk = 64;
template <int BITS>
__global__ void __launch_bounds__(1 << BITS) sort_scan1_kernel(const uint32_t *__restrict__ hist, int64_t nseg,
                                                               uint32_t *__restrict__ offs,
                                                               uint32_t *__restrict__ chunk_tot) {
  constexpr int NB = 1 << BITS;
  const int dgt = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * kScanChunk;
  const int64_t s1 = s0 + kScanChunk < nseg ? s0 + kScanChunk : nseg;
  uint32_t run = 0;
#pragma unroll 8
  for (int64_t sgm = s0; sgm < s1; ++sgm) {
    const uint32_t c = hist[sgm * NB + dgt];
    offs[sgm * NB + dgt] = run;
    run += c;
  }
  chunk_tot[(int64_t)blockIdx.x * NB + dgt] = run;
}
template <int BITS>
__global__ void __launch_bounds__(1 << BITS) sort_scan2_kernel(uint32_t *__restrict__ chunk_tot, int64_t nchunk) {
  constexpr int NB = 1 << BITS;
  __shared__ uint32_t tot[NB];
  const int dgt = threadIdx.x;
  uint32_t run = 0;
#pragma unroll 8
  for (int64_t c = 0; c < nchunk; ++c) {
    const uint32_t v = chunk_tot[c * NB + dgt];
    chunk_tot[c * NB + dgt] = run;
    run += v;
  }
  tot[dgt] = run;
  __syncthreads();
  uint32_t before = 0;
  for (int e = 0; e < dgt; ++e) before += tot[e];
#pragma unroll 8
  for (int64_t c = 0; c < nchunk; ++c) chunk_tot[c * NB + dgt] += before;
}

template <int BITS>
__global__ void __launch_bounds__(256) sort_scatter_kernel(const uint32_t *__restrict__ keys_in,
                                                           const uint32_t *__restrict__ vals_in, int64_t n,
                                                           int shift, const uint32_t *__restrict__ offs,
                                                           const uint32_t *__restrict__ chunk_base,
                                                           uint32_t *__restrict__ keys_out,
                                                           uint32_t *__restrict__ vals_out) {
  constexpr int NB = 1 << BITS;
  __shared__ uint32_t run[4][NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int64_t sgm = (int64_t)blockIdx.x * 4 + wave;
    for (int e = lane; e < NB; e += 64)
      run[wave][e] = offs[sgm * NB + e] + chunk_base[(sgm / kScanChunk) * NB + e];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int64_t base = (int64_t)blockIdx.x * kSortTile + wave * 1024;
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // the wave's 1024 keys and values: 32 unconditional loads (clamped index) issued up front -- loaded round by
  // round behind `i < n ? ... : 0`, each round paid its own memory round trip between two LDS synchronisations
  // (28 us per pass for 1.7 M keys)
  uint32_t kk[16], vv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t i = base + r * 64 + lane;
    kk[r] = keys_in[i < n ? i : n - 1];
    vv[r] = vals_in[i < n ? i : n - 1];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool ok = i < n;
    const uint32_t key = ok ? kk[r] : 0u;
    const uint32_t val = ok ? vv[r] : 0u;
    // inactive tail lanes get a digit of their own class so that they never rank among real keys
    const uint32_t digit = (key >> shift) & (uint32_t)(NB - 1);
    const uint64_t act = __ballot(ok);
    const uint64_t same = same_digit_mask<BITS>(digit) & act;
    if (ok) {
      const uint32_t rank = (uint32_t)__builtin_popcountll(same & below);
      const uint32_t dst = run[wave][digit] + rank;
      keys_out[dst] = key;
      vals_out[dst] = val;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (ok && (same & below) == 0ull) run[wave][digit] += (uint32_t)__builtin_popcountll(same);   // leader
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

static inline size_t sort_al(size_t x) { return (x + 255) / 256 * 256; }
}  // namespace tfrs

extern "C" size_t tfrs_embedding_scatter_add_workspace_bytes(int64_t n) {
  if (n <= 0) return 256;
  const size_t tiles = (size_t)((n + tfrs::kSortTile - 1) / tfrs::kSortTile);
  // (histograms and offsets of 4 waves x 1024 digits per tile, chunk totals of 1024 digits: the 10-bit passes)
  return 4 * tfrs::sort_al((size_t)n * 4) + 2 * tfrs::sort_al(tiles * 4096 * 4) +
         tfrs::sort_al((tiles * 4 / tfrs::kScanChunk + 1) * 1024 * 4);
}

// The sort's plan for a vocabulary: `passes` LSD passes of `digit_bits` (8, 9 or 10) bits each.  sort_id_positions
// launches exactly this plan (the exported function is the only place that computes it).
extern "C" int tfrs_embedding_sort_plan(int64_t vocab, int *passes_out, int *digit_bits_out) {
  TFRS_CHECK_ARG(vocab >= 1 && passes_out && digit_bits_out, "embedding_sort_plan: bad argument");
  // digits that can differ: the bits of vocab (0xFFFFFFFF of invalid ids needs the top pass too,
  // which the last valid pass provides as long as it covers a bit above vocab - 1)
  int bits = 1;
  while (bits < 32 && (1ll << bits) <= vocab) ++bits;   // 2^bits > vocab: invalid keys have bit `bits`.. set
  int passes = (bits + 1 + 7) / 8;
  if (passes > 4) passes = 4;
  // 9 or 10 bits per pass where that saves a whole pass (26 significant bits: 3 x 9; 28 .. 30: 3 x 10)
  int digit_bits = 8;
  for (int b = 9; b <= 10; ++b)
    if ((bits + 1 + b - 1) / b < passes) {
      passes = (bits + 1 + b - 1) / b;
      digit_bits = b;
    }
  *passes_out = passes;
  *digit_bits_out = digit_bits;
  return TFRS_OK;
}

// (declared in sparse_update.h: SortedPlan and ClippyAdagrad's two passes call it)
namespace tfrs {
int sort_id_positions(const void *ids, int ids_are_i64, int64_t n, int64_t vocab, void *workspace, hipStream_t s,
                      uint32_t *(&keys)[2], uint32_t *(&vals)[2]) {
  char *w = static_cast<char *>(workspace);
  const size_t kb = sort_al((size_t)n * 4);
  keys[0] = reinterpret_cast<uint32_t *>(w); keys[1] = reinterpret_cast<uint32_t *>(w + kb);
  vals[0] = reinterpret_cast<uint32_t *>(w + 2 * kb); vals[1] = reinterpret_cast<uint32_t *>(w + 3 * kb);
  const int64_t tiles = (n + kSortTile - 1) / kSortTile;
  uint32_t *hist = reinterpret_cast<uint32_t *>(w + 4 * kb);
  uint32_t *offs = reinterpret_cast<uint32_t *>(w + 4 * kb + sort_al((size_t)tiles * 4096 * 4));
  uint32_t *chunk = reinterpret_cast<uint32_t *>(w + 4 * kb + 2 * sort_al((size_t)tiles * 4096 * 4));
  const int64_t nseg = tiles * 4, nchunk = (nseg + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(sort_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, ids_are_i64, n,
                     vocab, keys[0], vals[0]);
  int passes = 0, digit_bits = 8;   // (a refused vocab -- every caller checks vocab >= 1 first -- sorts nothing)
  (void)tfrs_embedding_sort_plan(vocab, &passes, &digit_bits);
  int cur = 0;
  auto one_pass = [&](auto bc, int p) {
    constexpr int B = decltype(bc)::value;
    const int shift = B * p;
    hipLaunchKernelGGL(sort_hist_kernel<B>, dim3((unsigned)tiles), dim3(256), 0, s, keys[cur], n, shift, hist);
    hipLaunchKernelGGL(sort_scan1_kernel<B>, dim3((unsigned)nchunk), dim3(1 << B), 0, s, hist, nseg, offs, chunk);
    hipLaunchKernelGGL(sort_scan2_kernel<B>, dim3(1), dim3(1 << B), 0, s, chunk, nchunk);
    hipLaunchKernelGGL(sort_scatter_kernel<B>, dim3((unsigned)tiles), dim3(256), 0, s, keys[cur], vals[cur], n,
                       shift, offs, chunk, keys[cur ^ 1], vals[cur ^ 1]);
    cur ^= 1;
  };
  for (int p = 0; p < passes; ++p) {
    if (digit_bits == 10) one_pass(std::integral_constant<int, 10>{}, p);
    else if (digit_bits == 9) one_pass(std::integral_constant<int, 9>{}, p);
    else one_pass(std::integral_constant<int, 8>{}, p);
  }
  return cur;
}
}  // namespace tfrs

// ---- scatter-add (+ fused Adagrad) on the sorted route ---------------------------------------------------------------
// One lane per (position, chunk) over uint32 sorted keys / positions; keys >= vocab are the invalid / padding ids and
// sort last.
// NT: the gradient rows, the table / accumulator rows and their stores carry the non-temporal hint -- every one of them
// is touched once per launch, and a table beyond the last-level cache (the launcher asks for > 1 GiB) gains nothing from
// keeping them: 26 M x 128, 1.7 M ids, same box, alternating: 0.960 -> 0.933 ms (the loads alone 0.943, the stores alone +-0).
// LR: LrValue (the learning rate by value) or LrDevice (read once from the device float of tfrs_lr_tick), table_rules.h
namespace tfrs {
template <int VEC, bool NT = false, typename LR = LrValue>
__global__ void __launch_bounds__(256) scatter_add_u32_kernel(
    const float *__restrict__ grad_out, const uint32_t *__restrict__ sorted_ids,
    const uint32_t *__restrict__ perm, int64_t n, int d, uint32_t vocab, float *__restrict__ dst,
    float *__restrict__ accum, const LR lr_arg, float eps, int adagrad, int piece,
    const float *__restrict__ part) {
  const float lr = lr_arg.get();
  const int per_row = d / VEC;
  const SortedRuns runs = {grad_out, sorted_ids, perm, n, per_row, piece, part};
  const int64_t total = n * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per_row;
    const int c = (int)(t - i * per_row);
    // everything the common case (a run of one) needs goes out in TWO rounds of independent loads:
    // {id, its neighbours, the position} then {gradient piece, weights, accumulator}
    const uint32_t id = sorted_ids[i];
    const uint32_t id_prev = sorted_ids[i > 0 ? i - 1 : 0];          // (clamped: the loads are unconditional)
    const uint32_t id_next = sorted_ids[i + 1 < n ? i + 1 : n - 1];
    const int64_t src0 = perm[i];
    if (id >= vocab) continue;                       // invalid / padding id
    if (i > 0 && id_prev == id) continue;            // not the start of a run
    float g[VEC];
    float4 a_pre = make_float4(0.f, 0.f, 0.f, 0.f), w_pre = a_pre;
    if (VEC == 4 && adagrad) {
      const int64_t o4 = (int64_t)id * per_row + c;
      if (NT) {
        a_pre = nt_load4(reinterpret_cast<const float4 *>(accum) + o4);
        w_pre = nt_load4(reinterpret_cast<const float4 *>(dst) + o4);
      } else {
        a_pre = reinterpret_cast<const float4 *>(accum)[o4];
        w_pre = reinterpret_cast<const float4 *>(dst)[o4];
      }
    }
    runs.sum<VEC, NT>(i, id, id_next, src0, c, g);
    if (VEC == 4) {
      const int64_t o4 = (int64_t)id * per_row + c;
      float4 *d4 = reinterpret_cast<float4 *>(dst) + o4;
      if (adagrad) {
        float4 *a4 = reinterpret_cast<float4 *>(accum) + o4;
        float4 a = a_pre, w = w_pre;
        a.x += g[0] * g[0]; a.y += g[1 % VEC] * g[1 % VEC]; a.z += g[2 % VEC] * g[2 % VEC]; a.w += g[3 % VEC] * g[3 % VEC];
        w.x -= lr * g[0] / adagrad_denom(a.x, eps, adagrad); w.y -= lr * g[1 % VEC] / adagrad_denom(a.y, eps, adagrad);
        w.z -= lr * g[2 % VEC] / adagrad_denom(a.z, eps, adagrad); w.w -= lr * g[3 % VEC] / adagrad_denom(a.w, eps, adagrad);
        if (NT) {
          nt_store4(a, a4);
          nt_store4(w, d4);
        } else {
          *a4 = a;
          *d4 = w;
        }
      } else {
        *d4 = make_float4(g[0], g[1 % VEC], g[2 % VEC], g[3 % VEC]);
      }
    } else {
      const int64_t o = (int64_t)id * per_row + c;
      if (adagrad) {
        const float a = accum[o] + g[0] * g[0];
        accum[o] = a;
        dst[o] = dst[o] - lr * g[0] / adagrad_denom(a, eps, adagrad);
      } else {
        dst[o] = g[0];
      }
    }
  }
}

}  // namespace tfrs

// Backward of gather from UNSORTED ids: own radix sort + the segmented scatter-add / fused
// Adagrad above.  ids outside [0, vocab) are ignored (they read as zero rows in the forward).
extern "C" int tfrs_embedding_scatter_add_unsorted(const float *grad_out, const void *ids,
                                                   int ids_are_i64, int64_t n, int d, int64_t vocab,
                                                   float *grad_table_or_table, float *accum, float lr,
                                                   float eps, int adagrad, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
  return tfrs_embedding_scatter_add_unsorted_dlr(grad_out, ids, ids_are_i64, n, d, vocab, grad_table_or_table, accum,
                                                 lr, nullptr, eps, adagrad, workspace, workspace_bytes, stream);
}

// (lr_dev: NULL, or the device float of tfrs_lr_tick, read by the Adagrad epilogue in place of lr)
extern "C" int tfrs_embedding_scatter_add_unsorted_dlr(const float *grad_out, const void *ids,
                                                       int ids_are_i64, int64_t n, int d, int64_t vocab,
                                                       float *grad_table_or_table, float *accum, float lr,
                                                       const float *lr_dev, float eps, int adagrad, void *workspace,
                                                       size_t workspace_bytes, void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(n >= 0 && d >= 1 && vocab >= 1, "embedding_scatter_add_unsorted: bad shape");
  TFRS_CHECK_ARG(vocab < 0xFFFFFFFFll && n < 0xFFFFFFFFll,
                 "embedding_scatter_add_unsorted: vocab / n must fit 32 bits");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG(grad_out && ids && grad_table_or_table && workspace,
                 "embedding_scatter_add_unsorted: NULL pointer");
  TFRS_CHECK_ARG(!adagrad || accum, "embedding_scatter_add_unsorted: Adagrad needs an accumulator");
  if (workspace_bytes < tfrs_embedding_scatter_add_workspace_bytes(n)) {
    set_error("embedding_scatter_add_unsorted: workspace too small");
    return TFRS_ENOMEM;
  }
  const SortedPlan plan(ids, ids_are_i64, n, d, vocab, workspace, (hipStream_t)stream, grad_out,
                        (uintptr_t)grad_table_or_table | (uintptr_t)accum);
  TFRS_LAUNCH_CHECK();
  plan.pieces();
  auto launch = [&](auto lr_arg) {
    using LR = decltype(lr_arg);
#define TFRS_SCATTER_ADD(VEC, NT) \
  hipLaunchKernelGGL((scatter_add_u32_kernel<VEC, NT, LR>), plan.grid, dim3(256), 0, plan.s, grad_out, plan.keys, \
                     plan.vals, n, d, plan.vocab, grad_table_or_table, accum, lr_arg, eps, adagrad, plan.piece, plan.part)
    if (!plan.vec) TFRS_SCATTER_ADD(1, false);
    else if (plan.nt) TFRS_SCATTER_ADD(4, true);
    else TFRS_SCATTER_ADD(4, false);
#undef TFRS_SCATTER_ADD
  };
  if (lr_dev) launch(LrDevice{lr_dev});
  else launch(LrValue{lr});
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- the row scan's epilogues -------------------------------------------------------------------------------------------
// rowscan_sum (sparse_update.h) leaves every wave with its row's summed gradient; each optimizer adds its own epilogue on
// the touched rows.  Untouched rows are written by the plain scatter-add alone.
namespace tfrs {

// scatter-add (adagrad == 0: dst is the gradient table, untouched rows get their zeros here: no separate fill) or the
// fused Adagrad update
template <int NS>
__device__ __forceinline__ void rowscan_adagrad(const RowscanRow<NS> &r, int d, float *__restrict__ dst,
                                                float *__restrict__ accum, float lr, float eps, int adagrad) {
  if (!r.row_ok) return;
  if (adagrad) {
    if (r.touched) {   // wave-uniform
      float av[NS], pv[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        av[s] = accum[r.v * d + r.fo[s]];
        pv[s] = dst[r.v * d + r.fo[s]];
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (r.fok[s]) {
          const float a = av[s] + r.g[s] * r.g[s];
          accum[r.v * d + r.fo[s]] = a;
          dst[r.v * d + r.fo[s]] = pv[s] - lr * r.g[s] / adagrad_denom(a, eps, adagrad);
        }
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (r.fok[s]) dst[r.v * d + r.fo[s]] = r.g[s];
  }
}

// an update rule of table_rules.h: the touched rows of dst, slot0 and slot1 go through rule.apply
template <typename RULE, int NS>
__device__ __forceinline__ void rowscan_rule(const RowscanRow<NS> &r, int d, float *__restrict__ dst,
                                             float *__restrict__ slot0, float *__restrict__ slot1, const RULE &rule) {
  if (!(r.row_ok && r.touched)) return;   // wave-uniform
  float pv[NS], s0[NS], s1[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    pv[s] = dst[r.v * d + r.fo[s]];
    s0[s] = RULE::kSlots >= 1 ? slot0[r.v * d + r.fo[s]] : 0.0f;
    s1[s] = RULE::kSlots >= 2 ? slot1[r.v * d + r.fo[s]] : 0.0f;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (r.fok[s]) {
      rule.apply(r.g[s], pv[s], s0[s], s1[s]);
      dst[r.v * d + r.fo[s]] = pv[s];
      if (RULE::kSlots >= 1) slot0[r.v * d + r.fo[s]] = s0[s];
      if (RULE::kSlots >= 2) slot1[r.v * d + r.fo[s]] = s1[s];
    }
  }
}

// optimizers.RowWiseAdagrad: accum is ONE float per row, `mode` the denominator's; the row-wise functions of
// table_rules.h on the wave that already owns the row
template <int NS>
__device__ __forceinline__ void rowscan_rowwise(const RowscanRow<NS> &r, int d, float *__restrict__ dst,
                                                float *__restrict__ accum, float lr, float eps, int mode) {
  if (!(r.row_ok && r.touched)) return;   // wave-uniform
  float pv[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) pv[s] = dst[r.v * d + r.fo[s]];
  const float a_old = r.lane == 0 ? accum[r.v] : 0.0f;
  float partial = 0.0f;     // features lane, lane + 64, ... in ascending order, then the butterfly over the wave
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (r.fok[s]) partial = rowwise_sq_add(partial, r.g[s]);
  const float sum_sq = rowwise_group_sum(partial, 64);
  float scale = 0.0f;
  if (r.lane == 0) {
    const float a_new = rowwise_accumulate(a_old, sum_sq, d);
    accum[r.v] = a_new;
    scale = rowwise_scale(a_new, lr, eps, mode);
  }
  scale = __shfl(scale, 0);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (r.fok[s]) dst[r.v * d + r.fo[s]] = rowwise_step(pv[s], scale, r.g[s]);
}

// ClippyAdagrad on the touched rows: the factor pass (APPLY = false: min into *factor_slot) or the apply pass
template <bool APPLY, int NS>
__device__ __forceinline__ void rowscan_clippy(const RowscanRow<NS> &r, int d, float *__restrict__ dst,
                                               float *__restrict__ accum, float *__restrict__ factor_slot,
                                               const ClippyHyper &h) {
  const float factor = APPLY ? *factor_slot : 1.0f;
  float m = 1.0f;
  if (r.row_ok && r.touched) {   // wave-uniform
    float av[NS], pv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      av[s] = accum[r.v * d + r.fo[s]];
      pv[s] = dst[r.v * d + r.fo[s]];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (r.fok[s]) {
        const ClippyElement e = clippy_element(pv[s], av[s], r.g[s], h);
        if (APPLY) {
          clippy_apply(e, r.g[s], factor, h, pv[s], av[s]);
          accum[r.v * d + r.fo[s]] = av[s];
          dst[r.v * d + r.fo[s]] = pv[s];
        } else {
          m = clippy_min_scale(m, e);
        }
      }
    }
  }
  if (!APPLY) {
    m = clippy_wave_min(m);
    if (r.lane == 0) clippy_factor_min(factor_slot, m);
  }
}

// ---- scatter-add / Adagrad on the row scan ---------------------------------------------------------------------------
template <typename IdT>
__device__ __forceinline__ void scatter_rowscan_body(
    const float *__restrict__ grad_out, const void *__restrict__ ids, int64_t n, int d,
    int64_t vocab, float *__restrict__ dst, float *__restrict__ accum, float lr, float eps,
    int adagrad, int64_t block, int32_t *s_ids, int *s_hits) {
  TFRS_ROWSCAN_NS(d, rowscan_adagrad(rowscan_sum<IdT, NS>(grad_out, ids, n, d, vocab, block, s_ids, s_hits), d, dst, accum, lr, eps, adagrad));
}

template <typename IdT, typename LR = LrValue>
__global__ void __launch_bounds__(256) scatter_rowscan_kernel(
    const float *__restrict__ grad_out, const void *__restrict__ ids, int64_t n, int d,
    int64_t vocab, float *__restrict__ dst, float *__restrict__ accum, const LR lr_arg, float eps,
    int adagrad) {
  __shared__ int32_t s_ids[kRowscanChunk];
  __shared__ int s_hits[4 * kRowscanHitCap];
  const float lr = lr_arg.get();
  scatter_rowscan_body<IdT>(grad_out, ids, n, d, vocab, dst, accum, lr, eps, adagrad, blockIdx.x, s_ids, s_hits);
}

// Several small tables in ONE launch (the user and item tables of a two-tower step): each table's
// scan is a chain of dependent latencies (ids -> hits -> gradient rows -> row update), so two
// launches back to back cost twice the chain while one launch overlaps them.
struct RowscanTables {
  int ntab;
  int first_block[9];          // table t owns blocks [first_block[t], first_block[t + 1])
  const float *grad_out[8];
  const void *ids[8];
  int64_t n[8];
  int d[8];
  int64_t vocab[8];
  float *dst[8];
  float *accum[8];
  int i64[8];
};
template <typename LR = LrValue>
__global__ void __launch_bounds__(256) scatter_rowscan_multi_kernel(const RowscanTables t, const LR lr_arg, float eps,
                                                                    int adagrad) {
  const float lr = lr_arg.get();
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (i < t.ntab && (int)blockIdx.x >= t.first_block[i]) k = i;
  const int64_t block = (int)blockIdx.x - t.first_block[k];
  __shared__ int32_t s_ids[kRowscanChunk];
  __shared__ int s_hits[4 * kRowscanHitCap];
  if (t.i64[k])
    scatter_rowscan_body<int64_t>(t.grad_out[k], t.ids[k], t.n[k], t.d[k], t.vocab[k], t.dst[k], t.accum[k], lr,
                                  eps, adagrad, block, s_ids, s_hits);
  else
    scatter_rowscan_body<int32_t>(t.grad_out[k], t.ids[k], t.n[k], t.d[k], t.vocab[k], t.dst[k], t.accum[k], lr,
                                  eps, adagrad, block, s_ids, s_hits);
}

}  // namespace tfrs

extern "C" int tfrs_embedding_scatter_add_rowscan_multi(int ntables, const float *const *grad_out_h,
                                                        const void *const *ids_h,
                                                        const int *ids_are_i64_h, const int64_t *n_h,
                                                        const int *d_h, const int64_t *vocab_h,
                                                        float *const *tables_h, float *const *accum_h,
                                                        float lr, float eps, int adagrad,
                                                        void *stream) {
  return tfrs_embedding_scatter_add_rowscan_multi_dlr(ntables, grad_out_h, ids_h, ids_are_i64_h, n_h, d_h, vocab_h,
                                                      tables_h, accum_h, lr, nullptr, eps, adagrad, stream);
}

extern "C" int tfrs_embedding_scatter_add_rowscan_multi_dlr(int ntables, const float *const *grad_out_h,
                                                            const void *const *ids_h,
                                                            const int *ids_are_i64_h, const int64_t *n_h,
                                                            const int *d_h, const int64_t *vocab_h,
                                                            float *const *tables_h, float *const *accum_h,
                                                            float lr, const float *lr_dev, float eps, int adagrad,
                                                            void *stream) {
  TFRS_CHECK_ARG(ntables >= 1 && ntables <= 8, "embedding_scatter_add_rowscan_multi: 1..8 tables");
  TFRS_CHECK_ARG(grad_out_h && ids_h && ids_are_i64_h && n_h && d_h && vocab_h && tables_h,
                 "embedding_scatter_add_rowscan_multi: NULL argument array");
  tfrs::RowscanTables t = {};
  t.ntab = ntables;
  int blocks = 0;
  for (int i = 0; i < ntables; ++i) {
    TFRS_CHECK_ARG(n_h[i] >= 0 && d_h[i] >= 1 && d_h[i] <= 256 && vocab_h[i] >= 1,
                   "embedding_scatter_add_rowscan_multi: bad shape of table %d", i);
    TFRS_CHECK_ARG(tables_h[i] && (n_h[i] == 0 || (grad_out_h[i] && ids_h[i])) && (!adagrad || (accum_h && accum_h[i])),
                   "embedding_scatter_add_rowscan_multi: NULL pointer for table %d", i);
    t.first_block[i] = blocks;
    blocks += (int)((vocab_h[i] + 3) / 4);
    t.grad_out[i] = grad_out_h[i]; t.ids[i] = ids_h[i]; t.n[i] = n_h[i]; t.d[i] = d_h[i];
    t.vocab[i] = vocab_h[i]; t.dst[i] = tables_h[i]; t.accum[i] = accum_h ? accum_h[i] : nullptr;
    t.i64[i] = ids_are_i64_h[i];
  }
  t.first_block[ntables] = blocks;
  if (lr_dev)
    hipLaunchKernelGGL(tfrs::scatter_rowscan_multi_kernel<tfrs::LrDevice>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, t, tfrs::LrDevice{lr_dev}, eps, adagrad);
  else
    hipLaunchKernelGGL(tfrs::scatter_rowscan_multi_kernel<tfrs::LrValue>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, t, tfrs::LrValue{lr}, eps, adagrad);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_embedding_scatter_add_rowscan(const float *grad_out, const void *ids,
                                                  int ids_are_i64, int64_t n, int d,
                                                  int64_t vocab, float *grad_table_or_table,
                                                  float *accum, float lr, float eps, int adagrad,
                                                  void *stream) {
  return tfrs_embedding_scatter_add_rowscan_dlr(grad_out, ids, ids_are_i64, n, d, vocab, grad_table_or_table, accum, lr,
                                                nullptr, eps, adagrad, stream);
}

extern "C" int tfrs_embedding_scatter_add_rowscan_dlr(const float *grad_out, const void *ids,
                                                      int ids_are_i64, int64_t n, int d,
                                                      int64_t vocab, float *grad_table_or_table,
                                                      float *accum, float lr, const float *lr_dev, float eps,
                                                      int adagrad, void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(n >= 0 && d >= 1 && vocab >= 1, "embedding_scatter_add_rowscan: bad shape");
  TFRS_CHECK_ARG(d <= 256, "embedding_scatter_add_rowscan: d=%d > 256 (use the sorted path)", d);
  TFRS_CHECK_ARG((n == 0 || (grad_out && ids)) && grad_table_or_table,
                 "embedding_scatter_add_rowscan: NULL pointer");
  TFRS_CHECK_ARG(!adagrad || accum, "embedding_scatter_add_rowscan: Adagrad needs an accumulator");
  const dim3 grid((unsigned)((vocab + 3) / 4)), block(256);
  auto launch = [&](auto lr_arg) {
    using LR = decltype(lr_arg);
    if (ids_are_i64)
      hipLaunchKernelGGL((scatter_rowscan_kernel<int64_t, LR>), grid, block, 0, (hipStream_t)stream, grad_out, ids, n, d, vocab, grad_table_or_table, accum, lr_arg, eps, adagrad);
    else
      hipLaunchKernelGGL((scatter_rowscan_kernel<int32_t, LR>), grid, block, 0, (hipStream_t)stream, grad_out, ids, n, d, vocab, grad_table_or_table, accum, lr_arg, eps, adagrad);
  };
  if (lr_dev) launch(LrDevice{lr_dev});
  else launch(LrValue{lr});
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- ClippyAdagrad on the looked-up rows of a table (experimental/optimizers/clippy_adagrad.py:188-254 on IndexedSlices) ----
// The factor is the min over the TOUCHED rows (the reference gathers variable and accumulator at the indices), after
// duplicates are summed.  Two passes (clippy.h) over the same id structure: the row scan for small tables (rowscan_sum with
// rowscan_clippy), or ONE sort and two segmented passes.  The summed rows are RECOMPUTED in the apply pass, not kept: the same loads added in the
// same order give the same bits, it needs no [n, d] workspace (870 MB at 1.7 M x 128), and re-reading the gradient rows
// (n d 4 bytes) costs no more than writing and re-reading their sums would.  A run of equal ids is summed by one
// thread strictly in occurrence order -- not cut into parallel pieces like SortedRuns::sum's: the factor's
// error bound is stated against the sequential f32 sum.
namespace tfrs {

template <int VEC, bool APPLY, typename HYPER = ClippyHyper>
__global__ void __launch_bounds__(256) clippy_sorted_kernel(
    const float *__restrict__ grad_out, const uint32_t *__restrict__ sorted_ids, const uint32_t *__restrict__ perm,
    int64_t n, int d, uint32_t vocab, float *__restrict__ table, float *__restrict__ accum,
    float *__restrict__ factor_slot, const HYPER h_arg) {
  const ClippyHyper h = h_arg.get();
  const int per_row = d / VEC;
  const int64_t total = n * per_row;
  const float factor = APPLY ? *factor_slot : 1.0f;
  float m = 1.0f;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per_row;
    const int c = (int)(t - i * per_row);
    const uint32_t id = sorted_ids[i];
    const uint32_t id_prev = sorted_ids[i > 0 ? i - 1 : 0];
    if (id >= vocab) continue;                       // invalid / padding id
    if (i > 0 && id_prev == id) continue;            // not the start of a run
    const int64_t o = ((int64_t)id * per_row + c) * VEC;
    float w[VEC], a[VEC], g[VEC];
    vec_load<VEC, false>(table + o, w);
    vec_load<VEC, false>(accum + o, a);
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] = 0.f;
    // the run's first position, then eight positions per round: their gradient pieces are independent loads (a
    // position beyond the run re-reads the first piece and is dropped), added in occurrence order -- one memory latency
    // per eight duplicates instead of one per duplicate
    auto piece = [&](int64_t pos, float (&r)[VEC]) __attribute__((always_inline)) {
      vec_load<VEC, false>(grad_out + ((int64_t)perm[pos] * per_row + c) * VEC, r);
    };
    {
      float r[VEC];
      piece(i, r);
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] += r[v];
    }
    for (int64_t p = i + 1; p < n && sorted_ids[p] == id; p += 8) {
      float r[8][VEC];
      bool in_run[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        in_run[u] = p + u < n && sorted_ids[p + u < n ? p + u : p] == id;
        piece(in_run[u] ? p + u : i, r[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (in_run[u]) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) g[v] += r[u][v];
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const ClippyElement e = clippy_element(w[v], a[v], g[v], h);
      if (APPLY) clippy_apply(e, g[v], factor, h, w[v], a[v]);
      else m = clippy_min_scale(m, e);
    }
    if (APPLY) {
      vec_store<VEC, false>(table + o, w);
      vec_store<VEC, false>(accum + o, a);
    }
  }
  if (!APPLY) {
    m = clippy_wave_min(m);
    if ((threadIdx.x & 63) == 0) clippy_factor_min(factor_slot, m);
  }
}

template <typename IdT, bool APPLY, typename HYPER = ClippyHyper>
__global__ void __launch_bounds__(256) clippy_rowscan_kernel(
    const float *__restrict__ grad_out, const void *__restrict__ ids, int64_t n, int d, int64_t vocab,
    float *__restrict__ table, float *__restrict__ accum, float *__restrict__ factor_slot, const HYPER h_arg) {
  __shared__ int32_t s_ids[kRowscanChunk];
  __shared__ int s_hits[4 * kRowscanHitCap];
  const ClippyHyper h = h_arg.get();
  TFRS_ROWSCAN_NS(d, rowscan_clippy<APPLY>(rowscan_sum<IdT, NS>(grad_out, ids, n, d, vocab, blockIdx.x, s_ids, s_hits), d, table, accum, factor_slot, h));
}

}  // namespace tfrs

extern "C" size_t tfrs_clippy_sparse_workspace_bytes(int64_t n, int rowscan) {
  return rowscan ? 256 : tfrs_embedding_scatter_add_workspace_bytes(n);
}

extern "C" int tfrs_clippy_sparse(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d,
                                  int64_t vocab, float *table, float *accum, float *factor, float lr, float eps,
                                  float var_rel, float acc_rel, float abs_thr, int mode, int rowscan,
                                  void *workspace, size_t workspace_bytes, void *stream) {
  return tfrs_clippy_sparse_dlr(grad_out, ids, ids_are_i64, n, d, vocab, table, accum, factor, lr, nullptr, eps, var_rel,
                                acc_rel, abs_thr, mode, rowscan, workspace, workspace_bytes, stream);
}

extern "C" int tfrs_clippy_sparse_dlr(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d,
                                      int64_t vocab, float *table, float *accum, float *factor, float lr,
                                      const float *lr_dev, float eps, float var_rel, float acc_rel, float abs_thr,
                                      int mode, int rowscan, void *workspace, size_t workspace_bytes, void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(n >= 0 && d >= 1 && vocab >= 1, "clippy_sparse: bad shape");
  TFRS_CHECK_ARG(vocab < 0xFFFFFFFFll && n < 0xFFFFFFFFll, "clippy_sparse: vocab / n must fit 32 bits");
  TFRS_CHECK_ARG(table && accum && factor, "clippy_sparse: NULL pointer");
  TFRS_CHECK_ARG(mode >= 0 && mode <= 2, "clippy_sparse: mode must be 0 (delayed), 1 (delayed, clipped) or 2 (standard)");
  TFRS_CHECK_ARG(var_rel >= 0.f && acc_rel >= 0.f && abs_thr >= 0.f, "clippy_sparse: thresholds must be non-negative");
  TFRS_CHECK_ARG(!rowscan || d <= 256, "clippy_sparse: d=%d > 256 on the row-scan route (use the sorted route)", d);
  hipStream_t s = (hipStream_t)stream;
  const ClippyHyper h = {lr, eps, var_rel, acc_rel, abs_thr, mode};
  hipLaunchKernelGGL(clippy_arm_kernel, dim3(1), dim3(64), 0, s, factor, 1);
  if (n == 0) {     // factor 1, nothing written
    TFRS_LAUNCH_CHECK();
    return TFRS_OK;
  }
  TFRS_CHECK_ARG(grad_out && ids, "clippy_sparse: NULL pointer");
  if (rowscan) {
    const dim3 grid((unsigned)((vocab + 3) / 4)), block(256);
    auto launch = [&](auto ha) {
      using H = decltype(ha);
      if (ids_are_i64) {
        hipLaunchKernelGGL((clippy_rowscan_kernel<int64_t, false, H>), grid, block, 0, s, grad_out, ids, n, d, vocab, table, accum, factor, ha);
        hipLaunchKernelGGL((clippy_rowscan_kernel<int64_t, true, H>), grid, block, 0, s, grad_out, ids, n, d, vocab, table, accum, factor, ha);
      } else {
        hipLaunchKernelGGL((clippy_rowscan_kernel<int32_t, false, H>), grid, block, 0, s, grad_out, ids, n, d, vocab, table, accum, factor, ha);
        hipLaunchKernelGGL((clippy_rowscan_kernel<int32_t, true, H>), grid, block, 0, s, grad_out, ids, n, d, vocab, table, accum, factor, ha);
      }
    };
    if (lr_dev) launch(ClippyHyperDevice{h, lr_dev});
    else launch(h);
    TFRS_LAUNCH_CHECK();
    return TFRS_OK;
  }
  TFRS_CHECK_ARG(workspace, "clippy_sparse: NULL workspace");
  if (workspace_bytes < tfrs_embedding_scatter_add_workspace_bytes(n)) {
    set_error("clippy_sparse: workspace too small");
    return TFRS_ENOMEM;
  }
  // (the sort half of the plan only: the runs are summed whole, without pieces)
  const SortedPlan plan(ids, ids_are_i64, n, d, vocab, workspace, s, grad_out, (uintptr_t)table | (uintptr_t)accum);
  TFRS_LAUNCH_CHECK();
  auto launch = [&](auto ha) {
    using H = decltype(ha);
#define TFRS_CLIPPY_SORTED(VEC, APPLY) \
  hipLaunchKernelGGL((clippy_sorted_kernel<VEC, APPLY, H>), plan.grid, dim3(256), 0, s, grad_out, plan.keys, plan.vals, n, \
                     d, plan.vocab, table, accum, factor, ha)
    if (plan.vec) {
      TFRS_CLIPPY_SORTED(4, false);
      TFRS_CLIPPY_SORTED(4, true);
    } else {
      TFRS_CLIPPY_SORTED(1, false);
      TFRS_CLIPPY_SORTED(1, true);
    }
#undef TFRS_CLIPPY_SORTED
  };
  if (lr_dev) launch(ClippyHyperDevice{h, lr_dev});
  else launch(h);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// ---- optimizers.SGD / Adam / Ftrl on the looked-up rows of a table (table_rules.h) ----------------------------------
// The sparse Adagrad update with the arithmetic taken out: the same sort, the same piece-wise sums of long runs
// (scatter_add_pieces_kernel), the same two rounds of independent loads, the same row scan for small tables -- the rule
// is a template parameter, so the kernels below exist once.  A run's summed gradient is the one of the Adagrad
// kernels (SortedRuns::sum / rowscan_sum: the same code); a touched row
// whose sum is exactly zero is still updated (Adam's moments decay, Ftrl re-solves the row).
namespace tfrs {

template <typename RULE, int VEC, bool NT>
__global__ void __launch_bounds__(256) table_update_sorted_kernel(
    const float *__restrict__ grad_out, const uint32_t *__restrict__ sorted_ids, const uint32_t *__restrict__ perm,
    int64_t n, int d, uint32_t vocab, float *__restrict__ table, float *__restrict__ slot0, float *__restrict__ slot1,
    const RULE rule_arg, int piece, const float *__restrict__ part) {
  const RULE rule = rule_arg.resolved();
  const int per_row = d / VEC;
  const SortedRuns runs = {grad_out, sorted_ids, perm, n, per_row, piece, part};
  const int64_t total = n * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per_row;
    const int c = (int)(t - i * per_row);
    // round one: {id, its neighbours, the position}; round two: {gradient piece, weights, slots}
    const uint32_t id = sorted_ids[i];
    const uint32_t id_prev = sorted_ids[i > 0 ? i - 1 : 0];          // (clamped: the loads are unconditional)
    const uint32_t id_next = sorted_ids[i + 1 < n ? i + 1 : n - 1];
    const int64_t src0 = perm[i];
    if (id >= vocab) continue;                       // invalid / padding id: can never write
    if (i > 0 && id_prev == id) continue;            // not the start of a run
    const int64_t o = ((int64_t)id * per_row + c) * VEC;
    float w[VEC], s0[VEC], s1[VEC], g[VEC];
    vec_load<VEC, NT>(table + o, w);
#pragma unroll
    for (int v = 0; v < VEC; ++v) s0[v] = s1[v] = 0.f;
    if (RULE::kSlots >= 1) vec_load<VEC, NT>(slot0 + o, s0);
    if (RULE::kSlots >= 2) vec_load<VEC, NT>(slot1 + o, s1);
    runs.sum<VEC, NT>(i, id, id_next, src0, c, g);
#pragma unroll
    for (int v = 0; v < VEC; ++v) rule.apply(g[v], w[v], s0[v], s1[v]);
    vec_store<VEC, NT>(table + o, w);
    if (RULE::kSlots >= 1) vec_store<VEC, NT>(slot0 + o, s0);
    if (RULE::kSlots >= 2) vec_store<VEC, NT>(slot1 + o, s1);
  }
}

template <typename RULE, typename IdT>
__global__ void __launch_bounds__(256) table_update_rowscan_kernel(
    const float *__restrict__ grad_out, const void *__restrict__ ids, int64_t n, int d, int64_t vocab,
    float *__restrict__ table, float *__restrict__ slot0, float *__restrict__ slot1, const RULE rule_arg) {
  __shared__ int32_t s_ids[kRowscanChunk];
  __shared__ int s_hits[4 * kRowscanHitCap];
  const RULE rule = rule_arg.resolved();
  TFRS_ROWSCAN_NS(d, rowscan_rule(rowscan_sum<IdT, NS>(grad_out, ids, n, d, vocab, blockIdx.x, s_ids, s_hits), d, table, slot0, slot1, rule));
}

struct SparseUpdateArgs {
  const float *grad_out;
  const void *ids;
  int ids_are_i64;
  int64_t n;
  int d;
  int64_t vocab;
  float *table, *slot0, *slot1;
  int rowscan;
  void *workspace;
  hipStream_t stream;
};

template <typename RULE>
static int table_update_sparse_launch(const SparseUpdateArgs &a, const RULE &rule) {
  hipStream_t s = a.stream;
  const dim3 block(256);
  if (a.rowscan) {
    const dim3 grid((unsigned)((a.vocab + 3) / 4));
    if (a.ids_are_i64)
      hipLaunchKernelGGL((table_update_rowscan_kernel<RULE, int64_t>), grid, block, 0, s, a.grad_out, a.ids, a.n, a.d, a.vocab, a.table, a.slot0, a.slot1, rule);
    else
      hipLaunchKernelGGL((table_update_rowscan_kernel<RULE, int32_t>), grid, block, 0, s, a.grad_out, a.ids, a.n, a.d, a.vocab, a.table, a.slot0, a.slot1, rule);
    TFRS_LAUNCH_CHECK();
    return TFRS_OK;
  }
  const SortedPlan plan(a.ids, a.ids_are_i64, a.n, a.d, a.vocab, a.workspace, s, a.grad_out,
                        (uintptr_t)a.table | (uintptr_t)a.slot0 | (uintptr_t)a.slot1);
  TFRS_LAUNCH_CHECK();
  plan.pieces();
#define TFRS_TABLE_UPDATE_SORTED(VEC, NT) \
  hipLaunchKernelGGL((table_update_sorted_kernel<RULE, VEC, NT>), plan.grid, block, 0, s, a.grad_out, plan.keys, plan.vals, \
                     a.n, a.d, plan.vocab, a.table, a.slot0, a.slot1, rule, plan.piece, plan.part)
  if (!plan.vec) TFRS_TABLE_UPDATE_SORTED(1, false);
  else if (plan.nt) TFRS_TABLE_UPDATE_SORTED(4, true);
  else TFRS_TABLE_UPDATE_SORTED(4, false);
#undef TFRS_TABLE_UPDATE_SORTED
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

}  // namespace tfrs

extern "C" size_t tfrs_table_update_workspace_bytes(int64_t n, int rowscan) {
  return rowscan ? 256 : tfrs_embedding_scatter_add_workspace_bytes(n);
}

extern "C" int tfrs_table_update_sparse(int rule, const float *hyper_h, const float *alpha, const float *grad_out,
                                        const void *ids, int ids_are_i64, int64_t n, int d, int64_t vocab, float *table,
                                        float *slot0, float *slot1, int rowscan, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  using namespace tfrs;
  int rc = table_rule_check("table_update_sparse", rule, hyper_h, alpha);
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(n >= 0 && d >= 1 && vocab >= 1, "table_update_sparse: bad shape");
  TFRS_CHECK_ARG(vocab < 0xFFFFFFFFll && n < 0xFFFFFFFFll, "table_update_sparse: vocab / n must fit 32 bits");
  TFRS_CHECK_ARG(table && (rule == kRuleSgd || (slot0 && slot1)), "table_update_sparse: NULL pointer");
  TFRS_CHECK_ARG(!rowscan || d <= 256, "table_update_sparse: d=%d > 256 on the row-scan route (use the sorted route)", d);
  if (n == 0) return TFRS_OK;     // nothing is written
  TFRS_CHECK_ARG(grad_out && ids, "table_update_sparse: NULL pointer");
  if (!rowscan) {
    TFRS_CHECK_ARG(workspace, "table_update_sparse: NULL workspace");
    if (workspace_bytes < tfrs_embedding_scatter_add_workspace_bytes(n)) {
      set_error("table_update_sparse: workspace too small");
      return TFRS_ENOMEM;
    }
  }
  const SparseUpdateArgs a = {grad_out, ids, ids_are_i64, n, d, vocab, table, slot0, slot1, rowscan, workspace,
                              (hipStream_t)stream};
  // (for SGD and Ftrl a non-NULL alpha is the device floats of tfrs_lr_tick)
  if (rule == kRuleSgd) return table_update_sparse_launch(a, SgdRule{hyper_h[0], alpha});
  if (rule == kRuleAdam) return table_update_sparse_launch(a, AdamRule{hyper_h[0], hyper_h[1], hyper_h[2], alpha});
  if (hyper_h[4] != 0.0f) return table_update_sparse_launch(a, FtrlRule<true>{hyper_h[0], hyper_h[1], hyper_h[2], hyper_h[3], alpha});
  return table_update_sparse_launch(a, FtrlRule<false>{hyper_h[0], hyper_h[1], hyper_h[2], hyper_h[3], alpha});
}

// ---- optimizers.RowWiseAdagrad on the looked-up rows of a table (table_rules.h: one accumulator scalar per row) ------
// The same sort and the same piece-wise sums of long runs as every other sparse update (SortedPlan, SortedRuns::sum), but the rule needs the whole row's sum of
// squares before any element moves, so the thread layout differs from table_update_sorted_kernel: every sorted
// POSITION owns a group of 2^group_shift lanes (the power of two >= d / VEC, at most 64: a group never straddles a
// wave), only the groups of run starts work, and rowwise_adagrad_row does the rest -- a lane keeps its chunk of the
// summed gradient in registers, the group reduces the squares across lanes, one lane reads and writes acc[id] and
// divides, all lanes apply the scale to the G they still hold.  Rows wider than one chunk per lane (REREAD: d > 256
// on the float4 path, d > 64 on the scalar one) read and sum the gradient a SECOND time for the step instead of
// keeping several chunks per lane; the weights are read and written once either way.
namespace tfrs {

template <int VEC, bool REREAD, bool NT, typename LR>
__global__ void __launch_bounds__(256) rowwise_adagrad_sorted_kernel(
    const float *__restrict__ grad_out, const uint32_t *__restrict__ sorted_ids, const uint32_t *__restrict__ perm,
    int64_t n, int d, uint32_t vocab, float *__restrict__ table, float *__restrict__ accum, const LR lr_arg, float eps,
    int mode, int piece, const float *__restrict__ part, int group_shift) {
  const float lr = lr_arg.get();
  const int per_row = d / VEC;
  const SortedRuns runs = {grad_out, sorted_ids, perm, n, per_row, piece, part};
  const int group = 1 << group_shift;
  const int sub = (int)threadIdx.x & (group - 1);
  const int64_t total = n << group_shift;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t >> group_shift;      // (uniform over the group: its lanes leave or stay together)
    const uint32_t id = sorted_ids[i];
    const uint32_t id_prev = sorted_ids[i > 0 ? i - 1 : 0];          // (clamped: the loads are unconditional)
    const uint32_t id_next = sorted_ids[i + 1 < n ? i + 1 : n - 1];
    const int64_t src0 = perm[i];
    if (id >= vocab) continue;                       // invalid / padding id: can never write
    if (i > 0 && id_prev == id) continue;            // not the start of a run
    auto grad = [&](int c, float (&g)[VEC]) __attribute__((always_inline)) { runs.sum<VEC, NT>(i, id, id_next, src0, c, g); };
    rowwise_adagrad_row<VEC, REREAD, NT>(sub, group, per_row, d, table + (int64_t)id * d, accum + id, lr, eps, mode,
                                         grad);
  }
}

// The row scan with the row-wise epilogue (rowscan_rowwise): a wave already owns a row.
template <typename IdT, typename LR>
__global__ void __launch_bounds__(256) rowwise_adagrad_rowscan_kernel(
    const float *__restrict__ grad_out, const void *__restrict__ ids, int64_t n, int d, int64_t vocab,
    float *__restrict__ table, float *__restrict__ accum, const LR lr_arg, float eps, int mode) {
  __shared__ int32_t s_ids[kRowscanChunk];
  __shared__ int s_hits[4 * kRowscanHitCap];
  const float lr = lr_arg.get();
  TFRS_ROWSCAN_NS(d, rowscan_rowwise(rowscan_sum<IdT, NS>(grad_out, ids, n, d, vocab, blockIdx.x, s_ids, s_hits), d, table, accum, lr, eps, mode));
}

template <typename LR>
static int rowwise_adagrad_sparse_launch(const SparseUpdateArgs &a, const LR &lr, float eps, int mode) {
  hipStream_t s = a.stream;
  const dim3 block(256);
  if (a.rowscan) {
    const dim3 grid((unsigned)((a.vocab + 3) / 4));
    if (a.ids_are_i64)
      hipLaunchKernelGGL((rowwise_adagrad_rowscan_kernel<int64_t, LR>), grid, block, 0, s, a.grad_out, a.ids, a.n, a.d, a.vocab, a.table, a.slot0, lr, eps, mode);
    else
      hipLaunchKernelGGL((rowwise_adagrad_rowscan_kernel<int32_t, LR>), grid, block, 0, s, a.grad_out, a.ids, a.n, a.d, a.vocab, a.table, a.slot0, lr, eps, mode);
    TFRS_LAUNCH_CHECK();
    return TFRS_OK;
  }
  // (vec from the gradient and the table alone: the accumulator is one float per row)
  const SortedPlan plan(a.ids, a.ids_are_i64, a.n, a.d, a.vocab, a.workspace, s, a.grad_out, (uintptr_t)a.table);
  TFRS_LAUNCH_CHECK();
  plan.pieces();
  const int shift = rowwise_group_shift(plan.per_row);
  const bool reread = plan.per_row > 64;
  const dim3 grid(grid_for(a.n << shift, 256 * 64));     // a lane group per position
#define TFRS_ROWWISE_SORTED(VEC, REREAD, NT) \
  hipLaunchKernelGGL((rowwise_adagrad_sorted_kernel<VEC, REREAD, NT, LR>), grid, block, 0, s, a.grad_out, plan.keys, \
                     plan.vals, a.n, a.d, plan.vocab, a.table, a.slot0, lr, eps, mode, plan.piece, plan.part, shift)
  if (plan.vec) {
    if (reread) {
      if (plan.nt) TFRS_ROWWISE_SORTED(4, true, true);
      else TFRS_ROWWISE_SORTED(4, true, false);
    } else {
      if (plan.nt) TFRS_ROWWISE_SORTED(4, false, true);
      else TFRS_ROWWISE_SORTED(4, false, false);
    }
  } else {
    if (reread) TFRS_ROWWISE_SORTED(1, true, false);
    else TFRS_ROWWISE_SORTED(1, false, false);
  }
#undef TFRS_ROWWISE_SORTED
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

}  // namespace tfrs

// (lr_dev: NULL, or the device float of tfrs_lr_tick, read once at kernel entry in place of lr)
extern "C" int tfrs_rowwise_adagrad_sparse(const float *grad_out, const void *ids, int ids_are_i64, int64_t n, int d,
                                           int64_t vocab, float *table, float *accum, float lr, const float *lr_dev,
                                           float eps, int mode, int rowscan, void *workspace, size_t workspace_bytes,
                                           void *stream) {
  using namespace tfrs;
  TFRS_CHECK_ARG(mode == 1 || mode == 2, "rowwise_adagrad_sparse: mode must be 1 (sqrt(acc + eps)) or 2 (sqrt(acc) + eps)");
  TFRS_CHECK_ARG(n >= 0 && d >= 1 && vocab >= 1, "rowwise_adagrad_sparse: bad shape");
  TFRS_CHECK_ARG(vocab < 0xFFFFFFFFll && n < 0xFFFFFFFFll, "rowwise_adagrad_sparse: vocab / n must fit 32 bits");
  TFRS_CHECK_ARG(table && accum, "rowwise_adagrad_sparse: NULL pointer");
  TFRS_CHECK_ARG(eps >= 0.f, "rowwise_adagrad_sparse: epsilon must be non-negative");
  TFRS_CHECK_ARG(!rowscan || d <= 256, "rowwise_adagrad_sparse: d=%d > 256 on the row-scan route (use the sorted route)", d);
  if (n == 0) return TFRS_OK;     // nothing is written
  TFRS_CHECK_ARG(grad_out && ids, "rowwise_adagrad_sparse: NULL pointer");
  if (!rowscan) {
    TFRS_CHECK_ARG(workspace, "rowwise_adagrad_sparse: NULL workspace");
    if (workspace_bytes < tfrs_table_update_workspace_bytes(n, 0)) {
      set_error("rowwise_adagrad_sparse: workspace too small");
      return TFRS_ENOMEM;
    }
  }
  const SparseUpdateArgs a = {grad_out, ids, ids_are_i64, n, d, vocab, table, accum, nullptr, rowscan, workspace,
                              (hipStream_t)stream};
  if (lr_dev) return rowwise_adagrad_sparse_launch(a, LrDevice{lr_dev}, eps, mode);
  return rowwise_adagrad_sparse_launch(a, LrValue{lr}, eps, mode);
}

