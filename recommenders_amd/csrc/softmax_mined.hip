// softmax_mined.hip -- hard-negative mining, the softmax cross-entropy on the mined logits and the batch metric's
// rank count, all over ADJUSTED in-batch logits and without the [nq, nc] matrix (2-D queries).
//
// Replaces (tasks/retrieval.py) :178-203 (scores, temperature, SamplingProbablityCorrection,
// RemoveAccidentalHits, score_mask), HardNegativeMining :205-208 (layers/loss.py:91-109), the cross-entropy :210
// on the mined logits and in_top_k of the batch metrics :228-232.
//
//   S_bc  = (q_b . c_c) / T - corr_c  [+ MIN_FLOAT if ids_c == ids_b, c != b]  [= MIN_FLOAT where !mask_bc]
//           (IEEE f32 division, as the reference's scores / temperature; -0 -> +0)            (mined_logit)
//   keep(b, c) = (c == b) || S_bc > tau_b || (S_bc == tau_b && c <= cut_b)
//   tau_b = the n-th largest negative logit of row b, cut_b = the column of the last tied negative taken
//           (INT64_MAX: every tie at tau_b is taken) -- top_k's lower-column-first rule
//   loss  = sum_b w_b (logsumexp_{c : keep} S_bc - S_bb)
//   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) / T   where keep(b, c) and not masked, else 0
//   count_b = #{c != b : keep(b, c) and S_bc > S_bb}
//
// Every kernel instantiates a tile loop of softmax_shared.h with the mined policy (mined_logit, mined_keep, the
// row's tau / cut): mined_scan_kernel is softmax_stream_queries with one consumer per mode -- the loss forward is
// the shared OnlineSoftmax, the selection's and the count's consumers are below -- and mined_bwd_kernel is
// softmax_bwd_body.  A wave owns 32 rows as the MFMA B operand and streams 32-row tiles of the other side; a logit
// exists only in an accumulator register.  keep() compares RECOMPUTED logits with tau for equality, so every kernel
// forms S_bc by the same tile_dot over the same fragments (the dc kernel swaps the operand roles: each product
// commutes and the k order is the same) and the same mined_logit.
//
// Selection (exact, fixed launch sequence, no host read-back, no float atomics): a radix select over the
// order-preserving uint32 image of S (f32_orderable), four 8-bit passes.  A pass re-scores the tiles; every
// negative whose key matches the prefix fixed so far bumps hist[row][digit] in LDS (row stride 257 words:
// equal digits of different rows fall into different banks -- in the first pass nearly all digits are equal),
// the non-zero bins are flushed with integer atomicAdd into hist[nq, 256].  mined_pick_kernel then walks a
// row's bins from the top, fixes the digit, lowers the remaining rank and zeroes the bins for the next pass.
// After pass four a row knows tau, how many ties exist and how many it takes.  Only a row that takes FEWER
// ties than exist needs a cut column (real inputs do that: every masked / accidental-hit logit is exactly
// MIN_FLOAT): one scoring pass stores per-(split, row) tie counts, one more finds the r-th tie in column order
// in the split that holds it.  Both exit wave-uniformly when no row of the wave needs a cut.
#include "softmax_shared.h"

namespace tfrs {

constexpr int kHistStride = 257;   // words per row of the LDS histogram
constexpr int64_t kCutAll = INT64_MAX;

struct MinedArgs {
  SoftmaxArgs s;         // operands, options, split plan, partial buffers; s.inv_t = 1 / t is the gradient factor only
  float t;               // the temperature: divides the dot product
  const float *tau;      // [nq] threshold per row, or NULL: keep everything
  const int64_t *cut;    // [nq] cut column per row (read only with tau)
  // selection state (workspace)
  uint32_t *hist;        // [nq, 256] bins of the current pass
  uint32_t *prefix;      // [nq] key bits fixed so far
  uint32_t *krem;        // [nq] rank still wanted among the keys that match the prefix; after pass four: ties taken
  uint32_t *need;        // [nq] 1: the row takes fewer ties than exist
  uint32_t *tiecnt;      // [nsplit, nq] ties per split
  float *tau_w;          // [nq] outputs of the selection
  int64_t *cut_w;
  int pass;              // 0 .. 3
  uint32_t *cnt_part;    // [nsplit, nq] rank-count partials
};

enum { kModeHist = 0, kModeTieCount = 1, kModeTieFind = 2, kModeFwd = 3, kModeCount = 4 };

__device__ __forceinline__ float mined_logit(float dot, int64_t query, int64_t cand, const MinedArgs &a,
                                             float corr_c, int64_t id_q, int64_t id_c, bool *masked) {
  float v = __fdiv_rn(dot, a.t);
  if (a.s.corr) v -= corr_c;
  if (a.s.ids && cand != query && id_c == id_q) v += kMinFloat;
  *masked = false;
  if (a.s.mask && !a.s.mask[query * a.s.nc + cand]) {
    v = kMinFloat;
    *masked = true;
  }
  return v + 0.0f;  // -0 -> +0: compares and keys like +0
}

__device__ __forceinline__ bool mined_keep(float v, int64_t query, int64_t cand, float tau, int64_t cut) {
  return cand == query || v > tau || (v == tau && cand <= cut);
}

// The policy (softmax_shared.h) of every kernel here; without tau every column is kept.
struct MinedPolicy {
  const MinedArgs &a;
  struct Row {
    float tau = -__builtin_inff();
    int64_t cut = kCutAll;
  };
  __device__ __forceinline__ float logit(float dot, int64_t query, int64_t cand, float corr_c, int64_t id_q,
                                         int64_t id_c, bool *masked) const {
    return mined_logit(dot, query, cand, a, corr_c, id_q, id_c, masked);
  }
  __device__ __forceinline__ Row row(int64_t query) const {
    Row r;
    if (a.tau) {
      r.tau = a.tau[query];
      r.cut = a.cut[query];
    }
    return r;
  }
  __device__ static __forceinline__ bool keep(float v, int64_t query, int64_t cand, Row r) {
    return mined_keep(v, query, cand, r.tau, r.cut);
  }
};

using MinedLane = QueryLane<MinedPolicy::Row>;

// kModeHist (ONE wave per workgroup): every negative whose key matches the prefix fixed so far bumps its digit's bin
// of the LDS histogram `lds` [32, kHistStride]; the non-zero bins are flushed into hist[nq, 256].
struct HistConsumer {
  const MinedArgs &a;
  uint32_t *lds;
  uint32_t prefix_r = 0;

  template <class Frag>
  __device__ __forceinline__ bool begin(const MinedLane &w, const Frag &) {
    for (int i = w.lane; i < 32 * kHistStride; i += 64) lds[i] = 0u;
    if (w.qvalid) prefix_r = a.prefix[w.query];
    __syncthreads();  // one wave per workgroup
    return true;
  }
  __device__ __forceinline__ void element(const MinedLane &w, int, int64_t cand, bool valid, float v) {
    const int shift = 24 - 8 * a.pass;
    const uint32_t key = f32_orderable(v);
    if (valid && cand != w.query && (((key ^ prefix_r) >> shift) >> 8) == 0u)
      atomicAdd(&lds[w.j * kHistStride + ((key >> shift) & 255u)], 1u);
  }
  __device__ __forceinline__ void tile_end(const MinedLane &, int64_t) {}
  __device__ __forceinline__ void finish(const MinedLane &w) {
    __syncthreads();
    for (int i = w.lane; i < 32 * 256; i += 64) {
      const int row = i >> 8, bin = i & 255;
      const uint32_t v = lds[row * kHistStride + bin];
      if (v != 0u && w.qb * 32 + row < a.s.nq) atomicAdd(&a.hist[(w.qb * 32 + row) * 256 + bin], v);
    }
  }
};

// The cut passes.  kModeTieCount: ties with tau per (split, row); kModeTieFind: the column of the r-th tie of a row,
// in the split that holds it.  The wave leaves when no row of it takes fewer ties than exist / has its r-th tie here.
template <bool FIND>
struct TieConsumer {
  const MinedArgs &a;
  uint32_t want = 0, running = 0, tiebits = 0;
  bool active = false;
  int64_t found = -1;

  template <class Frag>
  __device__ __forceinline__ bool begin(const MinedLane &w, const Frag &) {
    active = w.qvalid && a.need[w.query] != 0u;
    if constexpr (FIND) {
      if (active) {
        want = a.krem[w.query];
        for (int p = 0; p < w.sp; ++p) running += a.tiecnt[(int64_t)p * a.s.nq + w.query];
        const uint32_t mine = a.tiecnt[(int64_t)w.sp * a.s.nq + w.query];
        active = running < want && want <= running + mine;
      }
    }
    return __any(active);
  }
  __device__ __forceinline__ void element(const MinedLane &w, int r, int64_t cand, bool valid, float v) {
    if (valid && cand != w.query && v == w.row.tau) tiebits |= 1u << tile_row_of_reg(r, w.h);
  }
  __device__ __forceinline__ void tile_end(const MinedLane &, int64_t c0) {
    // a query's 32 candidates of the tile sit in its two lane halves: bit t of `full` = tile row t ties with tau
    const uint32_t full = tiebits | (uint32_t)__shfl_xor((int)tiebits, 32);
    const uint32_t pc = (uint32_t)__popc(full);
    if constexpr (FIND) {
      if (active && found < 0 && running + pc >= want) {
        uint32_t bits = full;
        for (uint32_t skip = want - running - 1u; skip > 0u; --skip) bits &= bits - 1u;
        found = c0 + (__ffs((int)bits) - 1);
      }
    }
    running += pc;
    tiebits = 0;
  }
  __device__ __forceinline__ void finish(const MinedLane &w) {
    if constexpr (FIND) {
      if (w.h == 0 && active && found >= 0) a.cut_w[w.query] = found;
    } else {
      if (w.h == 0 && w.qvalid) a.tiecnt[(int64_t)w.sp * a.s.nq + w.query] = running;
    }
  }
};

// kModeCount: the kept negatives strictly above the positive, per (split, row); split 0 also writes the positive.
struct CountConsumer {
  const MinedArgs &a;
  float pos = 0.0f;
  uint32_t count = 0;

  // the positive logit from the diagonal tile (this wave's queries against candidates qb*32 .. +31), by the
  // arithmetic of every other tile: it ties exactly with copies of itself
  template <int HALF>
  __device__ __forceinline__ bool begin(const MinedLane &w, const float (&bq)[HALF]) {
    const SoftmaxArgs &s = a.s;
    const bool vec_ok = (s.d == 2 * HALF) && ((((uintptr_t)s.q) | ((uintptr_t)s.c)) % 16 == 0);
    float ad[HALF];
    load_row_frag<2 * HALF>(ad, s.c, w.query, w.qvalid, s.d, w.h, vec_ok);  // nq <= nc: a query is a candidate row
    const f32x16 acc = tile_dot<2 * HALF>(ad, bq);
    float own = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (tile_row_of_reg(r, w.h) == w.j && w.qvalid) {
        bool masked;
        own = mined_logit(acc[r], w.query, w.query, a, s.corr ? s.corr[w.query] : 0.0f, w.id_q, w.id_q, &masked);
      }
    const float other = __shfl_xor(own, 32);
    pos = (((w.j >> 2) & 1) == w.h) ? own : other;  // tile row j lives in lane half (j >> 2) & 1
    return true;
  }
  __device__ __forceinline__ void element(const MinedLane &w, int, int64_t cand, bool valid, float v) {
    if (valid && cand != w.query && MinedPolicy::keep(v, w.query, cand, w.row) && v > pos) ++count;
  }
  __device__ __forceinline__ void tile_end(const MinedLane &, int64_t) {}
  __device__ __forceinline__ void finish(const MinedLane &w) {
    const uint32_t total = count + (uint32_t)__shfl_xor((int)count, 32);
    if (w.h == 0 && w.qvalid) {
      a.cnt_part[(int64_t)w.sp * a.s.nq + w.query] = total;
      if (w.sp == 0) a.s.ppos[w.query] = pos;
    }
  }
};

// Waves own 32 queries and stream the candidates of one split; MODE selects the consumer of a tile of logits.
// kModeHist runs with ONE wave per workgroup (its LDS histogram), the others with four.
template <int DP, int MODE>
__global__ void __launch_bounds__(256) mined_scan_kernel(const MinedArgs a) {
  const MinedPolicy pol{a};
  if constexpr (MODE == kModeHist) {
    __shared__ uint32_t hist_lds[32 * kHistStride];
    HistConsumer con{a, hist_lds};
    softmax_stream_queries<DP, false, 1>(a.s, pol, con);
  } else if constexpr (MODE == kModeFwd) {
    OnlineSoftmax<MinedPolicy> con;
    softmax_stream_queries<DP, false, 4>(a.s, pol, con);
  } else if constexpr (MODE == kModeCount) {
    CountConsumer con{a};
    softmax_stream_queries<DP, false, 4>(a.s, pol, con);
  } else {
    TieConsumer<MODE == kModeTieFind> con{a};
    softmax_stream_queries<DP, false, 4>(a.s, pol, con);
  }
}

// Arms the selection: zero bins, empty prefix, wanted rank n.  n = 0 keeps the positive alone: tau = +inf, cut = -1
// are written here and nothing else runs.
__global__ void __launch_bounds__(256) mined_init_kernel(const MinedArgs a, uint32_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n == 0u) {
    for (int64_t row = t0; row < a.s.nq; row += stride) {
      a.tau_w[row] = __builtin_inff();
      a.cut_w[row] = -1;
    }
    return;
  }
  for (int64_t i = t0; i < a.s.nq * 256; i += stride) a.hist[i] = 0u;
  for (int64_t row = t0; row < a.s.nq; row += stride) {
    a.prefix[row] = 0u;
    a.krem[row] = n;
  }
}

// One thread per row: the digit of this pass is the highest bin at which the wanted rank is reached; the bins are
// zeroed for the next pass (and the next call).  After the last pass: tau, whether a cut is needed, cut = all ties.
__global__ void __launch_bounds__(256) mined_pick_kernel(const MinedArgs a) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.s.nq) return;
  uint32_t *bins = a.hist + row * 256;
  uint32_t k = a.krem[row], cnt = 0u;
  int digit = 0;
  bool found = false;
  for (int b = 255; b >= 0; --b) {
    const uint32_t c = bins[b];
    bins[b] = 0u;
    if (!found) {
      if (k <= c) {
        digit = b;
        cnt = c;
        found = true;
      } else {
        k -= c;
      }
    }
  }
  const uint32_t prefix = a.prefix[row] | ((uint32_t)digit << (24 - 8 * a.pass));
  a.prefix[row] = prefix;
  a.krem[row] = k;
  if (a.pass == 3) {
    a.tau_w[row] = f32_from_orderable(prefix);
    a.need[row] = k < cnt ? 1u : 0u;
    a.cut_w[row] = kCutAll;
  }
}

// counts[b] = sum over splits of the partial counts, bit 31 for a non-finite positive (tfrs_rank_count_accumulate's
// convention, consumed by tfrs_topk_hits_update)
__global__ void __launch_bounds__(256) mined_count_reduce_kernel(const MinedArgs a, uint32_t *counts) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.s.nq) return;
  uint32_t total = 0u;
  for (int sp = 0; sp < a.s.nsplit; ++sp) total += a.cnt_part[(int64_t)sp * a.s.nq + row];
  counts[row] = (total & 0x7FFFFFFFu) | (nonfinite_bits(a.s.ppos[row]) << 31);
}

// softmax_bwd_kernel of the 2-D route with keep() applied to every recomputed logit.
template <int DP, bool ROWS_ARE_QUERIES>
__global__ void __launch_bounds__(256) mined_bwd_kernel(const MinedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem_mined[];
  softmax_bwd_body<DP, ROWS_ARE_QUERIES, false>(a.s, MinedPolicy{a}, smem_mined);
}

template <int DP, int MODE>
static void launch_scan(const MinedArgs &a, hipStream_t st) {
  const int64_t waves = ((a.s.nq + 31) / 32) * a.s.nsplit;
  if (MODE == kModeHist)
    hipLaunchKernelGGL((mined_scan_kernel<DP, MODE>), dim3((unsigned)waves), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((mined_scan_kernel<DP, MODE>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a);
}

template <int MODE>
static void scan(const MinedArgs &a, hipStream_t st) {
  for_padded_dim(a.s.d, [&](auto dp) { launch_scan<decltype(dp)::value, MODE>(a, st); });
}

template <int DP, bool RQ>
static void launch_mined_bwd(const MinedArgs &a, hipStream_t st) {
  const int64_t waves = ((RQ ? a.s.nq : a.s.nc) + 31) / 32 * a.s.nsplit;
  const size_t lds = (size_t)4 * 32 * (DP + 4) * sizeof(float);
  hipLaunchKernelGGL((mined_bwd_kernel<DP, RQ>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, st, a);
}

// One workspace serves the four calls (each uses it from the start): the selection's bins and per-row state, the
// count's partials, and the loss kernels' SoftmaxLayout (softmax_shared.h) at one head.
static size_t mined_bytes(int64_t nq, int64_t nc, int d) {
  const SoftmaxLayout L = softmax_layout(nq, 1, nc, d);
  const size_t select = al((size_t)nq * 256 * 4) + 3 * al((size_t)nq * 4) + al((size_t)L.nsq * nq * 4);
  const size_t count = al((size_t)L.nsq * nq * 4) + al((size_t)nq * 4);
  return std::max(std::max(select, L.fwd), std::max(L.bwd, count));
}

// s.inv_t = 1 / t; the query plan (the scans' and the dq kernel's) is set, the loss runners set their own
static MinedArgs mined_args(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w, float t,
                            const float *corr, const int64_t *ids, const uint8_t *mask, const float *tau,
                            const int64_t *cut) {
  MinedArgs a = {};
  a.s = softmax_args(q, c, nq, 1, nc, d, w, 1.0f / t, corr, ids, mask);
  const SoftmaxLayout L = softmax_layout(nq, 1, nc, d);
  a.s.nsplit = L.nsq; a.s.split_len = L.lenq;
  a.t = t; a.tau = tau; a.cut = cut;
  return a;
}

}  // namespace tfrs

using namespace tfrs;

static int mined_check(const float *q, const float *c, int64_t nq, int64_t nc, int d, float t, const void *tau,
                       const void *cut, const void *ws, size_t ws_bytes, const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1 && d >= 1, "%s: bad shape (nq=%lld, nc=%lld, d=%d)", who, (long long)nq,
                 (long long)nc, d);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(d <= TFRS_MAX_DIM, "%s: embedding dim=%d above %d", who, d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  TFRS_CHECK_ARG(t == t && t != 0.0f && t - t == 0.0f, "%s: temperature must be finite and non-zero", who);
  TFRS_CHECK_ARG((tau == nullptr) == (cut == nullptr), "%s: tau and cut come together (both NULL: keep everything)",
                 who);
  TFRS_CHECK_ARG(ws, "%s: NULL workspace", who);
  TFRS_CHECK_ARG(ws_bytes >= mined_bytes(nq, nc, d), "%s: workspace too small", who);
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_mined_workspace_bytes(int64_t nq, int64_t nc, int d) {
  if (nq < 1 || nc < nq || d < 1 || d > TFRS_MAX_DIM) return 256;
  return mined_bytes(nq, nc, d);
}

extern "C" int tfrs_inbatch_mined_plan(int64_t nq, int64_t nc, int64_t *out) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= nq && out, "inbatch_mined_plan: bad argument");
  const SoftmaxLayout L = softmax_layout(nq, 1, nc, 1);
  out[0] = L.nsq; out[1] = L.lenq; out[2] = L.nsc; out[3] = L.lenc;
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_select(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         float temperature, const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, int64_t num_hard_negatives, float *tau,
                                         int64_t *cut, void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_select";
  TFRS_CHECK_ARG(num_hard_negatives >= 0, "%s: num_hard_negatives=%lld is negative", who,
                 (long long)num_hard_negatives);
  TFRS_CHECK_ARG(tau && cut, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, nullptr, temperature, log_q_correction, cand_ids, score_mask, nullptr,
                           nullptr);
  char *p = static_cast<char *>(workspace);
  a.hist = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 256 * 4);
  a.prefix = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.krem = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.need = reinterpret_cast<uint32_t *>(p); p += al((size_t)nq * 4);
  a.tiecnt = reinterpret_cast<uint32_t *>(p);
  a.tau_w = tau; a.cut_w = cut;
  const int64_t n = std::min<int64_t>(num_hard_negatives, nc - 1);  // loss.py:91
  const unsigned row_blocks = (unsigned)((nq + 255) / 256);
  hipLaunchKernelGGL(mined_init_kernel, dim3((unsigned)std::min<int64_t>(nq, 2048)), dim3(256), 0, st, a, (uint32_t)n);
  TFRS_LAUNCH_CHECK();
  if (n == 0) return TFRS_OK;
  for (a.pass = 0; a.pass < 4; ++a.pass) {
    scan<kModeHist>(a, st);
    TFRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mined_pick_kernel, dim3(row_blocks), dim3(256), 0, st, a);
    TFRS_LAUNCH_CHECK();
  }
  a.pass = 0;
  a.tau = tau;  // the cut passes compare with the threshold just written
  a.cut = cut;
  scan<kModeTieCount>(a, st);
  TFRS_LAUNCH_CHECK();
  scan<kModeTieFind>(a, st);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_inbatch_mined_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         const float *sample_weight, float temperature,
                                         const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, const float *tau, const int64_t *cut,
                                         float *out_loss, float *out_lse, float *out_pos, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_ce_fwd";
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, sample_weight, temperature, log_q_correction, cand_ids, score_mask, tau,
                           cut);
  return softmax_run_fwd(a.s, out_loss, out_lse, out_pos, workspace, st, [&](auto) { scan<kModeFwd>(a, st); });
}

extern "C" int tfrs_inbatch_mined_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                         const float *sample_weight, float temperature,
                                         const float *log_q_correction, const int64_t *cand_ids,
                                         const uint8_t *score_mask, const float *tau, const int64_t *cut,
                                         const float *lse, const float *gloss, float *dq, float *dc, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_ce_bwd";
  TFRS_CHECK_ARG(lse && dq && dc, "%s: NULL pointer", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, sample_weight, temperature, log_q_correction, cand_ids, score_mask, tau,
                           cut);
  a.s.lse = lse; a.s.gloss = gloss;
  return softmax_run_bwd(a.s, dq, dc, workspace, st, [&](auto dp, auto rq) {
    launch_mined_bwd<decltype(dp)::value, decltype(rq)::value>(a, st);
  });
}

extern "C" int tfrs_inbatch_mined_rank_count(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                                             float temperature, const float *log_q_correction,
                                             const int64_t *cand_ids, const uint8_t *score_mask, const float *tau,
                                             const int64_t *cut, uint32_t *counts, void *workspace,
                                             size_t workspace_bytes, void *stream) {
  const char *who = "inbatch_mined_rank_count";
  TFRS_CHECK_ARG(counts, "%s: NULL output", who);
  int rc = mined_check(q, c, nq, nc, d, temperature, tau, cut, workspace, workspace_bytes, who);
  if (rc != TFRS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MinedArgs a = mined_args(q, c, nq, nc, d, nullptr, temperature, log_q_correction, cand_ids, score_mask, tau, cut);
  char *p = static_cast<char *>(workspace);
  a.cnt_part = reinterpret_cast<uint32_t *>(p); p += al((size_t)a.s.nsplit * nq * 4);
  a.s.ppos = reinterpret_cast<float *>(p);
  scan<kModeCount>(a, st);
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mined_count_reduce_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, a, counts);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
