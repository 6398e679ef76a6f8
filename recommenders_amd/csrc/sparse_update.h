// What the sparse optimizer updates of sparse_update.hip share, each written once.  The float4-or-scalar access to a
// chunk of a row is in row_access.h (vec_load / vec_store); here: the summed gradient of a run
// of equal ids on the sorted route (SortedRuns::sum) with its host side (SortedPlan: the sort, the piece sums, the
// grids), and the scan half of the row scan for small tables (rowscan_sum, TFRS_ROWSCAN_NS).  Every update kernel is
// one of these two sums followed by its own arithmetic, so "the same bits as the other optimizers' sums" holds because
// it is the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "row_access.h"

namespace tfrs {

// ---- the sorted route ------------------------------------------------------------------------------------------------
// (id, position) pairs sorted by id (sort_id_positions); a lane owns chunk c of the row of a run's FIRST position i.
// Long runs of one id (a hot item of a Zipf-distributed feature, a padding id) are cut at multiples of `piece` positions
// (the first cut at least `piece` positions into the run): scatter_add_pieces_kernel sums every piece that CONTINUES a
// run across such a boundary into part[boundary / piece] (in parallel), and sum() adds the run's own first piece and then
// those partial sums.  Without this the whole run is one thread's serial loop: 1.5 M gradients for one row took 580 ms,
// 1500 per row 1.8 ms instead of 0.4.
struct SortedRuns {
  const float *__restrict__ grad_out;
  const uint32_t *__restrict__ sorted_ids;
  const uint32_t *__restrict__ perm;
  int64_t n;
  int per_row;
  int piece;
  const float *__restrict__ part;

  // g = the summed gradient of chunk c of the run of `id` that starts at position i.  The caller has already loaded
  // id = sorted_ids[i], id_next = sorted_ids[min(i + 1, n - 1)] and src0 = perm[i] in its first round of independent
  // loads; the first gradient piece (NT: with the non-temporal hint) joins the caller's second round.
  template <int VEC, bool NT>
  __device__ __forceinline__ void sum(int64_t i, uint32_t id, uint32_t id_next, int64_t src0, int c,
                                      float (&sum_out)[VEC]) const {
    float g[VEC];     // (a local, copied out at the end: summing into the caller's array compiled to a longer slow path)
    {
      float r[VEC];
      vec_load<VEC, NT>(grad_out + (src0 * per_row + c) * VEC, r);
#pragma unroll
      for (int v = 0; v < VEC; ++v) g[v] = 0.f + r[v];   // (0 + x, not x: the sum of a run starts from +0 like the oracle's, -0 gradients included)
    }
    // the run's first piece: up to the first multiple of `piece` that is >= i + piece ...
    int64_t p = i + 1;
    const int64_t first_end = ((i + piece - 1) / piece + 1) * (int64_t)piece;
    if (p < n && id_next == id) {
      for (; p < n && p < first_end && sorted_ids[p] == id; ++p) {
        float r[VEC];
        vec_load<VEC, false>(grad_out + ((int64_t)perm[p] * per_row + c) * VEC, r);
#pragma unroll
        for (int v = 0; v < VEC; ++v) g[v] += r[v];
      }
    }
    // ... then the partial sums of the pieces that continue it (scatter_add_pieces_kernel)
    if (p == first_end) {
      for (int64_t b = first_end / piece; b * piece < n && sorted_ids[b * piece] == id; ++b) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) g[v] += part[((b - 1) * per_row + c) * VEC + v];
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) sum_out[v] = g[v];
  }
};

template <int VEC>
__global__ void __launch_bounds__(256) scatter_add_pieces_kernel(
    const float *__restrict__ grad_out, const uint32_t *__restrict__ sorted_ids,
    const uint32_t *__restrict__ perm, int64_t n, int d, uint32_t vocab, int piece,
    float *__restrict__ part) {
  const int per_row = d / VEC;
  const int64_t nslots = (n + piece - 1) / piece;
  const int64_t total = nslots * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / per_row;
    const int c = (int)(t - b * per_row);
    const int64_t j = b * piece;
    if (b == 0 || j >= n) continue;
    const uint32_t id = sorted_ids[j];
    // a piece starts here only for a run that began at least `piece` positions earlier (ids are
    // sorted: equal ends mean an equal stretch), so runs shorter than `piece` are still summed by
    // ONE thread in position order -- bit-identical to the sequential oracle
    if (id >= vocab || sorted_ids[j - piece] != id) continue;
    float g[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) g[v] = 0.f;
    const int64_t end = (j + piece < n) ? j + piece : n;
    for (int64_t p = j; p < end && sorted_ids[p] == id; ++p) {
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
    for (int v = 0; v < VEC; ++v) part[((b - 1) * per_row + c) * VEC + v] = g[v];   // slot b - 1: boundary 0 continues nothing
  }
}

// The sort alone (sparse_update.hip): (id, position) pairs of `ids` in `workspace`
// (tfrs_embedding_scatter_add_workspace_bytes(n)), stable, ids outside [0, vocab) last.  Returns the index `cur` of the
// sorted buffers: sorted ids = keys[cur], positions = vals[cur]; keys[cur ^ 1] (n uint32) is free.  (Not an export of the
// library.)
__attribute__((visibility("hidden"))) int sort_id_positions(const void *ids, int ids_are_i64, int64_t n, int64_t vocab, void *workspace, hipStream_t s,
                      uint32_t *(&keys)[2], uint32_t *(&vals)[2]);

// The host side of a sorted update: the constructor sorts; pieces() launches the piece sums.  `vec`: d % 4 == 0 and
// every pointer of `aligned` (ORed together by the caller: the gradient, the table, its slots) 16-byte aligned.
struct __attribute__((visibility("hidden"))) SortedPlan {     // (host code of sparse_update.hip, not an export of the library)
  hipStream_t s;
  const float *grad_out;
  int64_t n;
  int d;
  uint32_t vocab;
  uint32_t *keys, *vals;   // sorted ids and their original positions
  bool vec;
  int per_row;             // chunks per row: d / 4 or d
  dim3 grid;               // one thread per (position, chunk), for the kernels laid out that way
  bool nt;                 // the non-temporal row streams (see scatter_add_u32_kernel): float4 path, table > 1 GiB, TFRS_SCATTER_NT != 0
  int piece;
  float *part;
  dim3 pgrid;

  SortedPlan(const void *ids, int ids_are_i64, int64_t n, int d, int64_t vocab, void *workspace, hipStream_t s,
             const float *grad_out, uintptr_t aligned)
      : s(s), grad_out(grad_out), n(n), d(d), vocab((uint32_t)vocab) {
    uint32_t *k[2], *v[2];
    const int cur = sort_id_positions(ids, ids_are_i64, n, vocab, workspace, s, k, v);
    keys = k[cur];
    vals = v[cur];
    vec = (d % 4 == 0) && (((uintptr_t)grad_out | aligned) % 16 == 0);
    per_row = vec ? d / 4 : d;
    grid = dim3(grid_for(n * per_row, 256 * 64));
    const char *nte = option("TFRS_SCATTER_NT");
    nt = vec && vocab * (int64_t)d * 4 > (1ll << 30) && !(nte && nte[0] == '0');
    // pieces of `piece` >= d positions: slot b - 1 (b >= 1, b * piece < n) ends at b * d <= b * piece < n
    // floats, i.e. inside the n floats of the sort's free ping-pong key buffer
    piece = 32;
    while (piece < d) piece *= 2;
    part = reinterpret_cast<float *>(k[cur ^ 1]);
    pgrid = dim3(grid_for(((n + piece - 1) / piece) * per_row, 256 * 64));
  }

  void pieces() const {
    if (vec)
      hipLaunchKernelGGL((scatter_add_pieces_kernel<4>), pgrid, dim3(256), 0, s, grad_out, keys, vals, n, d, vocab, piece, part);
    else
      hipLaunchKernelGGL((scatter_add_pieces_kernel<1>), pgrid, dim3(256), 0, s, grad_out, keys, vals, n, d, vocab, piece, part);
  }
};

// ---- the row scan: scatter-add for SMALL vocabularies, one wave per table row -------------------------------------------
// No sort: wave v scans the id list 64 at a time (ballot), and for every position that holds
// id v -- in ascending position, i.e. occurrence order, the order of the sorted path and of
// the oracle -- adds that gradient row (lane = feature).  O(vocab * n / 64) wave-steps: used
// when vocab * n is small (the MovieLens-sized tables of BASELINE configs[0]), where it
// replaces a 40 us radix sort + zero-fill per table with one ~5 us kernel.
constexpr int kRowscanChunk = 4096;   // ids per LDS chunk (int32 in LDS: anything outside [0, 2^31) matches no row: -1)
constexpr int kRowscanHitCap = 128;

// What the scan leaves to an epilogue: wave v's row, whether it exists and was looked up, and per lane the summed
// gradient of features fo[s] = lane + 64 s (clamped: a lane beyond d re-reads the row's last feature and drops it, !fok[s]).
template <int NS>
struct RowscanRow {
  int64_t v;
  bool row_ok, touched;   // wave-uniform
  int lane;
  float g[NS];
  int fo[NS];
  bool fok[NS];
};

// NS = number of 64-feature groups of a row (d <= 64 * NS): a template parameter so that every load of the gradient-row
// fetch is unconditional -- a load under `if (lane + 64 s < d)` makes the number of loads in flight unknown to the
// compiler, which then waits for each one (the ISA of the runtime-d version: 176 loads, at most ONE in flight).
// (the LDS arrays are declared ONCE by the kernel: static __shared__ arrays inside the template would be allocated per
// instantiation -- six copies of 18 KB)
template <typename IdT, int NS>
__device__ __forceinline__ RowscanRow<NS> rowscan_sum(const float *__restrict__ grad_out, const void *__restrict__ ids,
                                                      int64_t n, int d, int64_t vocab, int64_t block, int32_t *s_ids,
                                                      int *s_hits) {
  // the id list goes through LDS in chunks shared by the workgroup's 4 rows, so a wave's scan
  // is 64 LDS reads per 4096 ids instead of 64 dependent global loads
  constexpr int kChunk = kRowscanChunk;
  constexpr int kHitCap = kRowscanHitCap;
  int *my_hits = s_hits + (threadIdx.x >> 6) * kHitCap;
  const int lane = threadIdx.x & 63;
  const int64_t v = block * 4 + (threadIdx.x >> 6);
  const bool row_ok = v < vocab;
  float g[NS];  // features lane, lane + 64, ...
#pragma unroll
  for (int s = 0; s < NS; ++s) g[s] = 0.0f;
  int fo[NS];   // clamped feature offsets (a lane beyond d re-reads the row's last feature and drops it)
  bool fok[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    fok[s] = lane + 64 * s < d;
    fo[s] = fok[s] ? lane + 64 * s : d - 1;
  }
  bool touched = false;
  for (int64_t c0 = 0; c0 < n; c0 += kChunk) {
    const int m = (int)((n - c0 < kChunk) ? (n - c0) : kChunk);
    __syncthreads();
    {
      // all 16 loads of a thread in flight before the first LDS write, unconditionally (clamped into the chunk): one
      // memory round trip per chunk
      int64_t t[kChunk / 256];
#pragma unroll
      for (int i = 0; i < kChunk / 256; ++i) {
        const int e = threadIdx.x + i * 256;
        t[i] = load_id<IdT>(ids, c0 + (e < m ? e : m - 1));
      }
#pragma unroll
      for (int i = 0; i < kChunk / 256; ++i) {
        const int e = threadIdx.x + i * 256;
        if (e < m) s_ids[e] = (t[i] >= 0 && t[i] <= 0x7FFFFFFFll) ? (int32_t)t[i] : -1;
      }
    }
    __syncthreads();
    if (!row_ok) continue;
    // Two phases per chunk: the scan only records where this row's id occurs (in order); the
    // gradient rows are then fetched eight at a time as independent loads and added in
    // occurrence order -- one memory latency per eight duplicates instead of one per duplicate.
    int nh = 0;   // wave-uniform
    auto flush = [&]() __attribute__((always_inline)) {
      for (int i0 = 0; i0 < nh; i0 += 8) {
        float rr[8][NS];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int hp = (i0 + u < nh) ? my_hits[i0 + u] : my_hits[i0];
          const float *row = grad_out + (c0 + hp) * d;
#pragma unroll
          for (int s = 0; s < NS; ++s) rr[u][s] = row[fo[s]];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < nh) {   // uniform
#pragma unroll
            for (int s = 0; s < NS; ++s) g[s] += rr[u][s];
          }
      }
      nh = 0;
    };
    for (int base = 0; base < m; base += 64) {
      const int p = base + lane;
      const bool hit = (p < m) && ((int64_t)s_ids[p] == v);
      const uint64_t mask = __ballot(hit);
      if (mask == 0ull) continue;
      touched = true;
      if (nh + 64 > kHitCap) flush();
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      if (hit) my_hits[nh + (int)below] = p;
      nh += (int)__popcll(mask);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    flush();
  }
  RowscanRow<NS> r = {v, row_ok, touched, lane};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    r.g[s] = g[s];
    r.fo[s] = fo[s];
    r.fok[s] = fok[s];
  }
  return r;
}

// STATEMENT with `NS` the constant for a row of d <= 256 features.  (A macro, not a function taking a generic lambda:
// the scan inlined through a lambda's call operator compiled to 10 more VGPRs in every row-scan kernel.)
#define TFRS_ROWSCAN_NS(d, STATEMENT)                     \
  do {                                                    \
    if ((d) <= 64) { constexpr int NS = 1; STATEMENT; }   \
    else if ((d) <= 128) { constexpr int NS = 2; STATEMENT; } \
    else { constexpr int NS = 4; STATEMENT; }             \
  } while (0)

}  // namespace tfrs
