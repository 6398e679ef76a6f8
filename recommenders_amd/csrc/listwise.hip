// listwise.hip -- listwise ranking losses (softmax, pairwise logistic, pairwise hinge, ListMLE) with their gradients,
// the two pairwise ones also with LambdaRank / LambdaLoss pair weights, the three pair-sum losses (ApproxNDCG, ApproxMRR,
// UniqueSoftmax), and the per-list ranking metrics (NDCG, DCG, MRR,
// hits, precision, recall, MAP, ARP, OPA: all that a step asks for out of one launch), on [nlists, len] label / score
// matrices (losses.py, metrics/listwise.py; formulas: DESIGN 4.24, 4.25, 4.26).
//
// Position i of a list is VALID iff label[i] >= 0 (-1 pads; a NaN label is not valid either).  Invalid positions are
// selected out when the list is loaded -- their score is replaced by 0 and never enters any arithmetic -- and their
// gradient is stored as +0.
//
// Work mapping.  A workgroup has 256 threads; a list belongs to a GROUP of G threads, G the smallest of
// {8, 16, 32, 64} that is >= len, or 256 for 65 <= len <= 1024 (then a thread owns up to four items i = t + 256 c).
// A workgroup therefore carries 32 / 16 / 8 / 4 / 1 lists: a 5-item list costs 8 lanes, not a workgroup.  A list lives
// in the workgroup's LDS (scores, labels, 64-bit sort keys, two ping-pong scan buffers: 32 KiB at G = 256, 8 KiB below)
// and in registers; nothing else is allocated, the backward recomputes everything from the two inputs.  Every loop
// bound depends on (len, G) only -- never on the data -- so the workgroup barriers are uniform.
//
// Summation orders (every output is a fixed function of (kind, len); no atomics anywhere):
//   group sum      a thread first adds its own items c = 0, 1, 2, 3 in that order; then a xor butterfly over the
//                  min(G, 64) lanes of the group (offsets G/2, ..., 1); for G = 256 the four wave sums are added as
//                  ((w0 + w1) + w2) + w3.
//   pairwise       item i's loss / gradient contribution is the sum over j = 0, 1, ..., len - 1 in that order, in the
//                  thread that owns i (so the contributions to one position are combined in one register); the
//                  list's loss is the group sum of those.
//   sort           bitonic network on P = the power of two >= len (>= G for G < 256) keys in LDS.  A key is
//                  (orderable(value) << 32) | ~position, sorted descending: value descending, ties by position
//                  ascending, a total order, so the result does not depend on the network.  Invalid slots hold key 0
//                  and sink to the end.
//   ListMLE        sorted by label.  lse_r (logsumexp of the scores at ranks >= r) is a Hillis-Steele suffix scan of
//                  (max, sum) pairs, combine((m1, a1), (m2, a2)) = (m, a1 exp(m1 - m) + a2 exp(m2 - m)), m = max, with
//                  distances 1, 2, 4, ... < P; the gradient's sum_{r <= t} exp(s_t - lse_r) = exp(s_t + q_t) with q_t the
//                  same scan of -lse_r in the prefix direction.  Both scans never leave the range of the scores.
//   softmax        max, sum of exp(s - max), sum of y (lse - s), sum of y: group sums.
//   NDCG           two sorts (by score: DCG, by label: IDCG); each a group sum over the ranks r < min(n, topn) of
//                  (2^y - 1) / log2(r + 2), the thread that holds sorted slot r = sub + G c adding its ranks c = 0 .. 3
//                  in that order.  Metrics kernel (listwise_metrics_kernel); so are the eight below.  Counts (R, c_r,
//                  P, C, the number of positive labels) are integers: exact, their order immaterial.
//   DCG            NDCG's numerator: the same terms, the same group sum.
//   MRR            an integer group sum (r* + 1 at the one slot with rel and c_r = 1, r < k), one conversion, one division.
//   hits           c_{k-1} as an integer group sum of rel over the slots r < k; no float arithmetic.
//   precision      the same c_{k-1}; one division of two converted integers.
//   recall         the same c_{k-1}; one division by R.
//   MAP            c_r by ballot + popcount in the wave plus the totals of the 64-rank chunks before it; a group sum
//                  over the relevant ranks r < k of float(c_r) / float(r + 1); one division by R.
//   ARP            two group sums over the sorted slots, y and y * float(r + 1); one division.
//   OPA            the pairwise walk on two integer counters per thread; integer group sums; one division.
//   lambda weights the pairwise walk above with every term multiplied by w_ij before it is added; separate
//                  kernels (listwise_lambda_kernel), the unweighted ones carry no trace of them.  A sort by score; the
//                  thread at sorted slot r scatters rank r + 1 and the discount D(r + 1) to its item's position.  When
//                  normalised, first a sort by label and IDCG as in NDCG: a group sum over the ranks
//                  r < min(n, topn).  Per position, once: gain (2^y - 1), divided by IDCG when normalised (0 when
//                  IDCG <= 0).  Gains, discounts, ranks and (smooth) the table u(delta) = |D0(delta) - D0(delta + 1)|
//                  live in the four scan buffers.  w_ij = |G_i - G_j| * |D_i - D_j|, or, smooth,
//                  |G_i - G_j| * ((1 - mu) * |D_i - D_j| + mu * u(|r_i - r_j|)), evaluated in that order.
//   pair sums      ApproxNDCG, ApproxMRR, UniqueSoftmax (listwise_pairsum_kernel; formulas: DESIGN 4.28): a first walk
//                  whose per-item result feeds a second one.  alpha = 1 / temperature arrives as a float.
//     soft rank    r_i = 1 + sum over j = 0, 1, ..., len - 1 (valid, j != i) in that order of sigma(alpha (s_j - s_i)), in
//                  the thread that owns i, starting from 1; sigma and sigma' from e = exp(-|x|): one expf, one division.
//     ApproxNDCG   IDCG as in NDCG (label sort, every rank); the list's loss is -(group sum of
//                  (2^y_i - 1) / log2(1 + r_i)) / IDCG.  c_i = (2^y_i - 1) / (((IDCG ln2) (1 + r_i)) (lg lg)), lg = log2(1 + r_i).
//     ApproxMRR    Y = group sum of y; the loss is -(group sum of y_i / r_i) / Y; c_i = y_i / ((Y r_i) r_i).
//                  Both: 0 (and every gradient +0) where IDCG, Y <= 0.  Backward: c to a scan buffer, a barrier, then
//                  g_k = alpha * sum over j = 0 .. len - 1 (valid, j != k) of (c_j - c_k) sigma'(alpha (s_k - s_j)).
//     UniqueSoftmax  t = alpha s to a scan buffer.  Item i: m_i = max of t_i and the t_j with y_j < y_i (a walk of
//                  compares), a_i = sum over j = 0 .. len - 1 (j == i or y_j < y_i) in that order of exp(t_j - m_i) >= 1,
//                  lse_i = m_i + log a_i: finite for any finite scores.  Loss: group sum of (2^y_i - 1) (lse_i - t_i).
//                  Backward: lse and 2^y - 1 to scan buffers, a barrier, then g_k = alpha * sum over j = 0 .. len - 1 of
//                  G_k (exp(t_k - lse_k) - 1) at j == k and G_j exp(t_k - lse_j) where y_j > y_k (arguments <= 0).
#include "common.h"

namespace tfrs {

constexpr int kLwThreads = 256;
constexpr int kLwMaxLen = TFRS_LISTWISE_MAX_LEN;
enum { kLwSoftmax = TFRS_LISTWISE_SOFTMAX, kLwPairLogistic = TFRS_LISTWISE_PAIRWISE_LOGISTIC,
       kLwPairHinge = TFRS_LISTWISE_PAIRWISE_HINGE, kLwListMle = TFRS_LISTWISE_LIST_MLE };

template <int G>
struct LwCfg {
  static constexpr int IPT = G == 256 ? 4 : 1;   // items per thread
  static constexpr int LPB = kLwThreads / G;     // lists per workgroup
  static constexpr int CAP = G * IPT;            // LDS slots of one list
  static constexpr int N = kLwThreads * IPT;     // LDS slots of the workgroup
};

template <int G>
struct LwShared {
  float s[LwCfg<G>::N];
  float y[LwCfg<G>::N];
  uint64_t key[LwCfg<G>::N];
  float m[2][LwCfg<G>::N];
  float a[2][LwCfg<G>::N];
  float red[4];
};

template <int G>
__device__ __forceinline__ float lw_sum(float v, float *red) {
  constexpr int W = G < 64 ? G : 64;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if constexpr (G == 256) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((red[0] + red[1]) + red[2]) + red[3];
  }
  return v;
}
template <int G>
__device__ __forceinline__ float lw_max(float v, float *red) {
  constexpr int W = G < 64 ? G : 64;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  if constexpr (G == 256) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
  return v;
}

// One list's view: registers of the owning threads + its LDS slots.
template <int G>
struct LwList {
  int sub;          // thread within the group
  int off;          // first LDS slot of the list
  bool active;      // the group has a list
  int64_t base;     // first element of the list in the matrices
  float yv[LwCfg<G>::IPT], sv[LwCfg<G>::IPT];
  bool valid[LwCfg<G>::IPT];
};

// Loads the list (invalid positions selected out: label -1, score 0) into registers and LDS; ends with a barrier.
template <int G>
__device__ __forceinline__ void lw_load(LwList<G> &l, LwShared<G> &sh, const float *__restrict__ labels,
                                        const float *__restrict__ scores, int64_t nlists, int len) {
  constexpr int IPT = LwCfg<G>::IPT;
  const int grp = threadIdx.x / G;
  l.sub = threadIdx.x % G;
  l.off = grp * LwCfg<G>::CAP;
  const int64_t list = (int64_t)blockIdx.x * LwCfg<G>::LPB + grp;
  l.active = list < nlists;
  l.base = list * len;
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    const int i = l.sub + G * c;
    float y = -1.0f, s = 0.0f;
    if (l.active && i < len) {
      y = labels[l.base + i];
      s = scores[l.base + i];
    }
    const bool v = y >= 0.0f;
    l.valid[c] = v;
    l.yv[c] = v ? y : -1.0f;
    l.sv[c] = v ? s : 0.0f;
    sh.y[l.off + i] = l.yv[c];
    sh.s[l.off + i] = l.sv[c];
  }
  __syncthreads();
}

// Bitonic sort, descending, of the P keys of every list of the workgroup (P: power of two, G <= P or P <= CAP).
template <int G>
__device__ __forceinline__ void lw_sort(const LwList<G> &l, LwShared<G> &sh, int P) {
  constexpr int IPT = LwCfg<G>::IPT;
  uint64_t *key = sh.key + l.off;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int i = l.sub + G * c;
        const int p = i ^ j;
        if (i < P && p > i) {
          const uint64_t a = key[i], b = key[p];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) {
            key[i] = b;
            key[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ void lw_combine(float m1, float a1, float m2, float a2, float &m, float &a) {
  m = fmaxf(m1, m2);
  if (m == -__builtin_inff()) {
    a = 0.0f;
    return;
  }
  a = a1 * expf(m1 - m) + a2 * expf(m2 - m);
}

// Inclusive logsumexp scan of the (m, a) pairs in buffer 0 over P slots; SUFFIX: slot t combines t, t + 1, ...;
// else t, t - 1, ....  Returns the buffer that holds the result.  Entry and exit: barrier done.
template <int G, bool SUFFIX>
__device__ __forceinline__ int lw_scan(const LwList<G> &l, LwShared<G> &sh, int P) {
  constexpr int IPT = LwCfg<G>::IPT;
  int cur = 0;
  for (int d = 1; d < P; d <<= 1) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int t = l.sub + G * c;
      if (t < P) {
        float m = sh.m[cur][l.off + t], a = sh.a[cur][l.off + t];
        const int p = SUFFIX ? t + d : t - d;
        if (p >= 0 && p < P) lw_combine(m, a, sh.m[cur][l.off + p], sh.a[cur][l.off + p], m, a);
        sh.m[cur ^ 1][l.off + t] = m;
        sh.a[cur ^ 1][l.off + t] = a;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  return cur;
}

__device__ __forceinline__ float lw_logistic(float x) { return fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float lw_logistic_grad(float x) {      // -1 / (1 + exp(x)) without overflow
  const float e = expf(-fabsf(x));
  return x >= 0.0f ? -e / (1.0f + e) : -1.0f / (1.0f + e);
}

// Sum over j of item i's pair terms (see the header): loss terms, or gradient terms when BWD.
template <int G, bool HINGE, bool BWD>
__device__ __forceinline__ void lw_pairs(const LwList<G> &l, const LwShared<G> &sh, int len, float *acc) {
  constexpr int IPT = LwCfg<G>::IPT;
#pragma unroll
  for (int c = 0; c < IPT; ++c) acc[c] = 0.0f;
  for (int j = 0; j < len; ++j) {
    const float yj = sh.y[l.off + j], sj = sh.s[l.off + j];
    if (!(yj >= 0.0f)) continue;
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      if (!l.valid[c]) continue;
      const float yi = l.yv[c], si = l.sv[c];
      if (yi > yj) {
        const float x = si - sj;
        if (BWD) acc[c] += HINGE ? (x < 1.0f ? -1.0f : 0.0f) : lw_logistic_grad(x);
        else acc[c] += HINGE ? fmaxf(0.0f, 1.0f - x) : lw_logistic(x);
      } else if (BWD && yj > yi) {
        const float x = sj - si;
        acc[c] -= HINGE ? (x < 1.0f ? -1.0f : 0.0f) : lw_logistic_grad(x);
      }
    }
  }
}

template <int G, bool BWD>
__global__ void __launch_bounds__(kLwThreads) listwise_loss_kernel(int kind, const float *__restrict__ labels,
                                                                   const float *__restrict__ scores, int64_t nlists,
                                                                   int len, int P, const float *__restrict__ scale,
                                                                   float *__restrict__ out) {
  constexpr int IPT = LwCfg<G>::IPT;
  __shared__ LwShared<G> sh;
  LwList<G> l;
  lw_load<G>(l, sh, labels, scores, nlists, len);
  const int64_t list = (int64_t)blockIdx.x * LwCfg<G>::LPB + threadIdx.x / G;
  const float sc = (BWD && l.active) ? scale[list] : 0.0f;
  float g[IPT];        // BWD: gradient of the item a thread owns (softmax, pairwise)
  float loss = 0.0f;   // !BWD: the list's loss

  if (kind == kLwSoftmax) {
    float t = -__builtin_inff();
#pragma unroll
    for (int c = 0; c < IPT; ++c) if (l.valid[c]) t = fmaxf(t, l.sv[c]);
    const float mx = lw_max<G>(t, sh.red);
    t = 0.0f;
#pragma unroll
    for (int c = 0; c < IPT; ++c) if (l.valid[c]) t += expf(l.sv[c] - mx);
    const float se = lw_sum<G>(t, sh.red);
    const float lse = mx + logf(se);                // n == 0: no valid item below reads it
    t = 0.0f;
    if (BWD) {
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (l.valid[c]) t += l.yv[c];
      const float ysum = lw_sum<G>(t, sh.red);
#pragma unroll
      for (int c = 0; c < IPT; ++c) g[c] = l.valid[c] ? ysum * expf(l.sv[c] - lse) - l.yv[c] : 0.0f;
    } else {
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (l.valid[c]) t += l.yv[c] * (lse - l.sv[c]);
      loss = lw_sum<G>(t, sh.red);
    }
  } else if (kind == kLwPairLogistic || kind == kLwPairHinge) {
    float acc[IPT];
    if (kind == kLwPairHinge) lw_pairs<G, true, BWD>(l, sh, len, acc);
    else lw_pairs<G, false, BWD>(l, sh, len, acc);
    if (BWD) {
#pragma unroll
      for (int c = 0; c < IPT; ++c) g[c] = acc[c];
    } else {
      float t = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) t += acc[c];
      loss = lw_sum<G>(t, sh.red);
    }
  } else {   // ListMLE
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      sh.key[l.off + i] = l.valid[c] ? make_key(l.yv[c], i) : 0ull;
    }
    __syncthreads();
    lw_sort<G>(l, sh, P);
    int pos[IPT];
    bool ok[IPT];
    float sp[IPT], lse[IPT];
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int t = l.sub + G * c;
      const uint64_t k = t < P ? sh.key[l.off + t] : 0ull;
      ok[c] = k != 0ull;
      pos[c] = ok[c] ? key_index(k) : 0;
      sp[c] = ok[c] ? sh.s[l.off + pos[c]] : 0.0f;
      if (t < P) {
        sh.m[0][l.off + t] = ok[c] ? sp[c] : -__builtin_inff();
        sh.a[0][l.off + t] = ok[c] ? 1.0f : 0.0f;
      }
    }
    __syncthreads();
    int buf = lw_scan<G, true>(l, sh, P);
    float t = 0.0f;
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int r = l.sub + G * c;
      lse[c] = ok[c] ? sh.m[buf][l.off + r] + logf(sh.a[buf][l.off + r]) : 0.0f;
      if (ok[c]) t += lse[c] - sp[c];
    }
    if (!BWD) {
      loss = lw_sum<G>(t, sh.red);
    } else {
      __syncthreads();
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int r = l.sub + G * c;
        if (r < P) {
          sh.m[0][l.off + r] = ok[c] ? -lse[c] : -__builtin_inff();
          sh.a[0][l.off + r] = ok[c] ? 1.0f : 0.0f;
        }
      }
      __syncthreads();
      buf = lw_scan<G, false>(l, sh, P);
      // padded positions first (+0), then every valid item at its own position: disjoint
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int i = l.sub + G * c;
        if (l.active && i < len && !l.valid[c]) out[l.base + i] = 0.0f;
      }
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int r = l.sub + G * c;
        if (l.active && ok[c]) {
          const float q = sh.m[buf][l.off + r] + logf(sh.a[buf][l.off + r]);
          out[l.base + pos[c]] = sc * (expf(sp[c] + q) - 1.0f);
        }
      }
    }
    if (BWD) return;
  }

  if (BWD) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      if (l.active && i < len) out[l.base + i] = l.valid[c] ? sc * g[c] : 0.0f;
    }
  } else if (l.active && l.sub == 0) {
    out[list] = loss;
  }
}

// ---- ranking metrics (NDCG, DCG, MRR, hits, precision, recall, MAP, ARP, OPA; formulas: DESIGN 4.26) ---------------------
// Every requested metric of a list out of ONE launch: the list is loaded once and sorted by score once (a second sort,
// by label, only when some metric is NDCG; the pair walk only when some metric is OPA).  What to compute arrives as a
// by-value descriptor -- a kernel argument, no device memory -- so every branch on it is uniform over the grid.
enum { kLmNdcg = TFRS_LISTWISE_METRIC_NDCG, kLmDcg = TFRS_LISTWISE_METRIC_DCG, kLmMrr = TFRS_LISTWISE_METRIC_MRR,
       kLmHits = TFRS_LISTWISE_METRIC_HITS, kLmPrecision = TFRS_LISTWISE_METRIC_PRECISION,
       kLmRecall = TFRS_LISTWISE_METRIC_RECALL, kLmMap = TFRS_LISTWISE_METRIC_MAP, kLmArp = TFRS_LISTWISE_METRIC_ARP,
       kLmOpa = TFRS_LISTWISE_METRIC_OPA };
enum { kLmLabelSort = 1,   // some NDCG: the ideal order
       kLmScoreSort = 2,   // anything but OPA
       kLmGain = 4,        // NDCG, DCG: the terms (2^y - 1) / log2(r + 2)
       kLmCount = 8,       // MRR, hits, precision, recall, MAP: rel, c_r, R
       kLmArpSums = 16, kLmPairs = 32,
       kLmPositive = 64 };   // DCG: its weight, [some label > 0]
struct LwMetricDesc {      // (ints only: the kernel copies it to LDS word by word)
  int n, flags;
  int rank_lim;   // the widest cut of the metrics that read the score order: no sorted slot beyond it is looked at
  int gain_lim;   // the widest cut of the NDCG / DCG metrics: no gain term is evaluated at a rank beyond it
  int kind[TFRS_LISTWISE_METRIC_MAX], topn[TFRS_LISTWISE_METRIC_MAX];
};

// lw_sum on integers (exact, so its order is immaterial); the wave sums cross LDS as bit patterns.
template <int G>
__device__ __forceinline__ int lw_isum(int v, float *red) {
  constexpr int W = G < 64 ? G : 64;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if constexpr (G == 256) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __int_as_float(v);
    __syncthreads();
    v = __float_as_int(red[0]) + __float_as_int(red[1]) + __float_as_int(red[2]) + __float_as_int(red[3]);
  }
  return v;
}

template <int G>
__global__ void __launch_bounds__(kLwThreads) listwise_metrics_kernel(const float *__restrict__ labels,
                                                                      const float *__restrict__ scores,
                                                                      float *__restrict__ values,
                                                                      float *__restrict__ weights, int64_t nlists,
                                                                      int len, int P, const LwMetricDesc d) {
  constexpr int IPT = LwCfg<G>::IPT;
  constexpr int kWords = sizeof(LwMetricDesc) / sizeof(int);
  __shared__ LwShared<G> sh;
  // The descriptor goes to LDS (a[1], free here) with the first loads of the kernel and is read from there: a
  // kernel-argument read at its point of use -- in the metric loop, after the sorts -- is a trip to the argument memory
  // that nothing overlaps, paid by every workgroup.  lw_load's barrier covers the copy.
  if (threadIdx.x < kWords) sh.a[1][threadIdx.x] = __int_as_float(reinterpret_cast<const int *>(&d)[threadIdx.x]);
  const float *dw = sh.a[1];
  LwList<G> l;
  lw_load<G>(l, sh, labels, scores, nlists, len);
  const int nmetrics = __float_as_int(dw[0]), flags = __float_as_int(dw[1]);
  const int rank_lim = __float_as_int(dw[2]), gain_lim = __float_as_int(dw[3]);
  // what the thread keeps of sorted slot r = sub + G c: ideal order (by label) and score order
  float ti[IPT], tr[IPT], yr[IPT];     // gain terms of the two orders; the label at score rank r
  bool oki[IPT], okr[IPT], rel[IPT];   // a valid item sits at the slot; it is relevant (y >= 1)
  int cr[IPT];                         // c_r: relevant items at score ranks <= r
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    ti[c] = tr[c] = 0.0f;
    yr[c] = -1.0f;
    oki[c] = okr[c] = rel[c] = false;
    cr[c] = 0;
  }

  if (flags & kLmLabelSort) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      sh.key[l.off + i] = l.valid[c] ? make_key(l.yv[c], i) : 0ull;
    }
    __syncthreads();
    lw_sort<G>(l, sh, P);
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int r = l.sub + G * c;
      const uint64_t k = r < P && r < gain_lim ? sh.key[l.off + r] : 0ull;
      oki[c] = k != 0ull;
      if (oki[c]) ti[c] = (exp2f(sh.y[l.off + key_index(k)]) - 1.0f) / log2f((float)(r + 2));
    }
    __syncthreads();
  }

  int nrel = 0, npos = 0;              // R; the number of valid labels > 0
  float ysum = 0.0f, ynum = 0.0f;      // ARP: sum_V y, sum_V y (r + 1)
  if (flags & kLmScoreSort) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      sh.key[l.off + i] = l.valid[c] ? make_key(l.sv[c], i) : 0ull;
    }
    __syncthreads();
    lw_sort<G>(l, sh, P);
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int r = l.sub + G * c;
      const uint64_t k = r < P && r < rank_lim ? sh.key[l.off + r] : 0ull;
      okr[c] = k != 0ull;
      if (okr[c]) {
        yr[c] = sh.y[l.off + key_index(k)];
        rel[c] = yr[c] >= 1.0f;
        if ((flags & kLmGain) && r < gain_lim) tr[c] = (exp2f(yr[c]) - 1.0f) / log2f((float)(r + 2));
      }
    }
    if (flags & kLmPositive) {
      int t = 0;
#pragma unroll
      for (int c = 0; c < IPT; ++c) t += l.valid[c] && l.yv[c] > 0.0f ? 1 : 0;
      npos = lw_isum<G>(t, sh.red);
    }
    if (flags & kLmCount) {
      // c_r: ballot + popcount inside the wave (a group of G < 64 lanes reads its own bits of the mask); at G = 256
      // slot r lies in 64-rank chunk 4 c + wave, and the 16 chunk totals cross LDS (in m[0], free here)
      const int lane = threadIdx.x & 63;
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const uint64_t mask = __ballot(rel[c]);
        if constexpr (G == 256) {
          cr[c] = __popcll(mask & ((2ull << lane) - 1ull));
          if (lane == 0) sh.m[0][4 * c + (threadIdx.x >> 6)] = __int_as_float(__popcll(mask));
        } else if constexpr (G == 64) {
          cr[c] = __popcll(mask & ((2ull << lane) - 1ull));
        } else {
          const uint64_t mine = (mask >> (lane / G * G)) & ((1ull << G) - 1ull);
          cr[c] = __popcll(mine & ((2ull << l.sub) - 1ull));
        }
      }
      if constexpr (G == 256) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < IPT; ++c) {
          const int q = 4 * c + (threadIdx.x >> 6);
          int before = 0;
#pragma unroll
          for (int p = 0; p < 4 * IPT - 1; ++p) before += p < q ? __float_as_int(sh.m[0][p]) : 0;
          cr[c] += before;
        }
      }
      int t = 0;
#pragma unroll
      for (int c = 0; c < IPT; ++c) t += l.valid[c] && l.yv[c] >= 1.0f ? 1 : 0;      // (own items: every rank counts)
      nrel = lw_isum<G>(t, sh.red);
    }
    if (flags & kLmArpSums) {
      float t = 0.0f, u = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        if (okr[c]) {
          t += yr[c];
          u += yr[c] * (float)(l.sub + G * c + 1);
        }
      }
      ysum = lw_sum<G>(t, sh.red);
      ynum = lw_sum<G>(u, sh.red);
    }
  }

  int npairs = 0, nright = 0;          // OPA: P and C
  if (flags & kLmPairs) {            // the broadcast j loop of lw_pairs, on integer counts
    int pc = 0, cc = 0;
    for (int j = 0; j < len; ++j) {
      const float yj = sh.y[l.off + j], sj = sh.s[l.off + j];
      if (!(yj >= 0.0f)) continue;
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        if (l.valid[c] && l.yv[c] > yj) {
          ++pc;
          cc += l.sv[c] > sj ? 1 : 0;
        }
      }
    }
    npairs = lw_isum<G>(pc, sh.red);
    nright = lw_isum<G>(cc, sh.red);
  }

  const int64_t list = (int64_t)blockIdx.x * LwCfg<G>::LPB + threadIdx.x / G;
  for (int m = 0; m < nmetrics; ++m) {
    const int kind = __float_as_int(dw[4 + m]), topn = __float_as_int(dw[4 + TFRS_LISTWISE_METRIC_MAX + m]);
    const int lim = topn > 0 && topn < P ? topn : P;      // rank r is inside the cut iff r < lim and a valid item is there
    float v = 0.0f, w = 0.0f;
    if (kind == kLmNdcg || kind == kLmDcg) {
      float t = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (okr[c] && l.sub + G * c < lim) t += tr[c];
      const float dcg = lw_sum<G>(t, sh.red);
      if (kind == kLmNdcg) {
        t = 0.0f;
#pragma unroll
        for (int c = 0; c < IPT; ++c) if (oki[c] && l.sub + G * c < lim) t += ti[c];
        const float idcg = lw_sum<G>(t, sh.red);
        const bool cnt = idcg > 0.0f;
        v = cnt ? dcg / idcg : 0.0f;
        w = cnt ? 1.0f : 0.0f;
      } else {
        w = npos > 0 ? 1.0f : 0.0f;
        v = npos > 0 ? dcg : 0.0f;
      }
    } else if (kind == kLmMrr) {
      int t = 0;                                           // r* + 1 at the one slot that holds the first relevant item
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (rel[c] && cr[c] == 1 && l.sub + G * c < lim) t += l.sub + G * c + 1;
      const int first = lw_isum<G>(t, sh.red);
      w = nrel > 0 ? 1.0f : 0.0f;
      v = first > 0 ? 1.0f / (float)first : 0.0f;
    } else if (kind == kLmHits || kind == kLmPrecision || kind == kLmRecall) {
      int t = 0;
#pragma unroll
      for (int c = 0; c < IPT; ++c) t += rel[c] && l.sub + G * c < lim ? 1 : 0;
      const int ck = lw_isum<G>(t, sh.red);                // c_{k - 1}
      w = nrel > 0 ? 1.0f : 0.0f;
      if (kind == kLmHits) v = ck > 0 ? 1.0f : 0.0f;
      else if (kind == kLmPrecision) v = (float)ck / (float)(topn > 0 && topn < len ? topn : len);
      else v = nrel > 0 ? (float)ck / (float)nrel : 0.0f;
    } else if (kind == kLmMap) {
      float t = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c)
        if (rel[c] && l.sub + G * c < lim) t += (float)cr[c] / (float)(l.sub + G * c + 1);
      const float ap = lw_sum<G>(t, sh.red);
      w = nrel > 0 ? 1.0f : 0.0f;
      v = nrel > 0 ? ap / (float)nrel : 0.0f;
    } else if (kind == kLmArp) {
      w = ysum > 0.0f ? ysum : 0.0f;
      v = ysum > 0.0f ? ynum / ysum : 0.0f;
    } else {   // OPA
      w = (float)npairs;
      v = npairs > 0 ? (float)nright / (float)npairs : 0.0f;
    }
    if (l.active && l.sub == 0) {
      values[(int64_t)m * nlists + list] = v;
      weights[(int64_t)m * nlists + list] = w;
    }
  }
}

// ---- lambda weights (LambdaRank / LambdaLoss pair weights on the DCG or NDCG gain) -----------------------
// The per-position quantities of the weights in the scan buffers, which the pairwise kinds leave free.
template <int G>
struct LwLambda {
  float *gain, *disc, *rank, *table;
  __device__ __forceinline__ LwLambda(LwShared<G> &sh, int off)
      : gain(sh.m[0] + off), disc(sh.m[1] + off), rank(sh.a[0] + off), table(sh.a[1] + off) {}
};

__device__ __forceinline__ float lw_discount(int r) { return 1.0f / log2f((float)(r + 1)); }   // D0(r), r = 1, 2, ...

// Fills the buffers of LwLambda for the loaded list: entry barrier done (lw_load), ends with a barrier.
template <int G, bool SMOOTH>
__device__ __forceinline__ void lw_lambda_prepare(const LwList<G> &l, LwShared<G> &sh, int P, int topn,
                                                  int normalized) {
  constexpr int IPT = LwCfg<G>::IPT;
  LwLambda<G> lam(sh, l.off);
  const int lim = topn > 0 && topn < P ? topn : P;
  float idcg = 1.0f;
  if (normalized) {                                   // (a kernel argument: uniform)
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      sh.key[l.off + i] = l.valid[c] ? make_key(l.yv[c], i) : 0ull;
    }
    __syncthreads();
    lw_sort<G>(l, sh, P);
    float t = 0.0f;
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int r = l.sub + G * c;
      const uint64_t k = r < lim ? sh.key[l.off + r] : 0ull;
      if (k != 0ull) t += (exp2f(sh.y[l.off + key_index(k)]) - 1.0f) / log2f((float)(r + 2));
    }
    idcg = lw_sum<G>(t, sh.red);
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    const int i = l.sub + G * c;
    sh.key[l.off + i] = l.valid[c] ? make_key(l.sv[c], i) : 0ull;
    float g = l.valid[c] ? exp2f(l.yv[c]) - 1.0f : 0.0f;
    if (normalized) g = idcg > 0.0f ? g / idcg : 0.0f;
    lam.gain[i] = g;
    lam.disc[i] = 0.0f;                               // (invalid positions: never read by a pair, but defined)
    lam.rank[i] = 0.0f;
    if (SMOOTH) lam.table[i] = i >= 1 ? fabsf(lw_discount(i) - lw_discount(i + 1)) : 0.0f;
  }
  __syncthreads();
  lw_sort<G>(l, sh, P);
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    const int r = l.sub + G * c;
    const uint64_t k = r < P ? sh.key[l.off + r] : 0ull;
    if (k != 0ull) {                                  // one sorted slot per valid position: disjoint writes
      const int pos = key_index(k);
      lam.disc[pos] = r < lim ? lw_discount(r + 1) : 0.0f;
      lam.rank[pos] = (float)(r + 1);
    }
  }
  __syncthreads();
}

// lw_pairs with every term multiplied by its pair weight.
template <int G, bool HINGE, bool BWD, bool SMOOTH>
__device__ __forceinline__ void lw_lambda_pairs(const LwList<G> &l, LwShared<G> &sh, int len, int topn, float mu,
                                                float *acc) {
  constexpr int IPT = LwCfg<G>::IPT;
  const LwLambda<G> lam(sh, l.off);
  const float cut = topn > 0 ? (float)topn : __builtin_inff();
  const float nu = 1.0f - mu;
  float gi[IPT], di[IPT], ri[IPT];
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    const int i = l.sub + G * c;
    acc[c] = 0.0f;
    gi[c] = lam.gain[i];
    di[c] = lam.disc[i];
    ri[c] = lam.rank[i];
  }
  for (int j = 0; j < len; ++j) {
    const float yj = sh.y[l.off + j], sj = sh.s[l.off + j];
    if (!(yj >= 0.0f)) continue;
    const float gj = lam.gain[j], dj = lam.disc[j];
    const float rj = SMOOTH ? lam.rank[j] : 0.0f;
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      if (!l.valid[c]) continue;
      const float yi = l.yv[c], si = l.sv[c];
      if (!(yi > yj) && !(BWD && yj > yi)) continue;
      float w = fabsf(di[c] - dj);
      if (SMOOTH) {
        const float u = lam.table[(int)fabsf(ri[c] - rj)];          // 1 <= |r_i - r_j| <= n - 1 < CAP
        w = fminf(ri[c], rj) > cut ? 0.0f : nu * w + mu * u;
      }
      w = fabsf(gi[c] - gj) * w;
      if (yi > yj) {
        const float x = si - sj;
        if (BWD) acc[c] += w * (HINGE ? (x < 1.0f ? -1.0f : 0.0f) : lw_logistic_grad(x));
        else acc[c] += w * (HINGE ? fmaxf(0.0f, 1.0f - x) : lw_logistic(x));
      } else {
        const float x = sj - si;
        acc[c] -= w * (HINGE ? (x < 1.0f ? -1.0f : 0.0f) : lw_logistic_grad(x));
      }
    }
  }
}

template <int G, bool BWD, bool SMOOTH>
__global__ void __launch_bounds__(kLwThreads) listwise_lambda_kernel(int kind, const float *__restrict__ labels,
                                                                     const float *__restrict__ scores, int64_t nlists,
                                                                     int len, int P, int topn, int normalized, float mu,
                                                                     const float *__restrict__ scale,
                                                                     float *__restrict__ out) {
  constexpr int IPT = LwCfg<G>::IPT;
  __shared__ LwShared<G> sh;
  LwList<G> l;
  lw_load<G>(l, sh, labels, scores, nlists, len);
  const int64_t list = (int64_t)blockIdx.x * LwCfg<G>::LPB + threadIdx.x / G;
  const float sc = (BWD && l.active) ? scale[list] : 0.0f;
  lw_lambda_prepare<G, SMOOTH>(l, sh, P, topn, normalized);
  float acc[IPT];
  if (kind == kLwPairHinge) lw_lambda_pairs<G, true, BWD, SMOOTH>(l, sh, len, topn, mu, acc);
  else lw_lambda_pairs<G, false, BWD, SMOOTH>(l, sh, len, topn, mu, acc);
  if (BWD) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      if (l.active && i < len) out[l.base + i] = l.valid[c] ? sc * acc[c] : 0.0f;
    }
  } else {
    float t = 0.0f;
#pragma unroll
    for (int c = 0; c < IPT; ++c) t += acc[c];
    const float loss = lw_sum<G>(t, sh.red);
    if (l.active && l.sub == 0) out[list] = loss;
  }
}

// ---- pair-sum losses (ApproxNDCG, ApproxMRR, UniqueSoftmax) ----------------------------------------------
// A walk over j whose per-item result (soft rank, restricted logsumexp) feeds a second walk over j: the per-position
// quantities of the second one cross the scan buffers, which these kinds leave free.
enum { kPsApproxNdcg = TFRS_LISTWISE_APPROX_NDCG, kPsApproxMrr = TFRS_LISTWISE_APPROX_MRR,
       kPsUniqueSoftmax = TFRS_LISTWISE_UNIQUE_SOFTMAX };
constexpr float kLwLn2 = 0.693147180559945309f;

// sigma(x) = 1 / (1 + exp(-x)) and sigma'(x) = sigma(x) sigma(-x) from e = exp(-|x|) <= 1: no overflow.
__device__ __forceinline__ float lw_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.0f ? 1.0f : e) / (1.0f + e);
}
__device__ __forceinline__ float lw_sigmoid_grad(float x) {
  const float e = expf(-fabsf(x)), d = 1.0f + e;
  return e / (d * d);
}

// r_i = 1 + sum_{j valid, j != i} sigma(alpha (s_j - s_i)) of the items a thread owns.
template <int G>
__device__ __forceinline__ void lw_soft_ranks(const LwList<G> &l, const LwShared<G> &sh, int len, float alpha, float *r) {
  constexpr int IPT = LwCfg<G>::IPT;
#pragma unroll
  for (int c = 0; c < IPT; ++c) r[c] = 1.0f;
  for (int j = 0; j < len; ++j) {
    const float yj = sh.y[l.off + j], sj = sh.s[l.off + j];
    if (!(yj >= 0.0f)) continue;
#pragma unroll
    for (int c = 0; c < IPT; ++c)
      if (l.valid[c] && l.sub + G * c != j) r[c] += lw_sigmoid(alpha * (sj - l.sv[c]));
  }
}

// lse_i = log(exp(t_i) + sum_{j valid, y_j < y_i} exp(t_j)) of the items a thread owns, t = the list's slots of a scan
// buffer: the maximum first (compares), then the sum of exp(t_j - m_i), which holds exp(0) and so is >= 1.
template <int G>
__device__ __forceinline__ void lw_unique_lse(const LwList<G> &l, const LwShared<G> &sh, int len, const float *t,
                                              float *ti, float *lse) {
  constexpr int IPT = LwCfg<G>::IPT;
  float m[IPT], a[IPT];
#pragma unroll
  for (int c = 0; c < IPT; ++c) {
    ti[c] = t[l.sub + G * c];
    m[c] = ti[c];
    a[c] = 0.0f;
  }
  for (int j = 0; j < len; ++j) {
    const float yj = sh.y[l.off + j], tj = t[j];
    if (!(yj >= 0.0f)) continue;
#pragma unroll
    for (int c = 0; c < IPT; ++c)
      if (l.valid[c] && yj < l.yv[c]) m[c] = fmaxf(m[c], tj);
  }
  for (int j = 0; j < len; ++j) {
    const float yj = sh.y[l.off + j], tj = t[j];
    if (!(yj >= 0.0f)) continue;
#pragma unroll
    for (int c = 0; c < IPT; ++c)
      if (l.valid[c] && (yj < l.yv[c] || l.sub + G * c == j)) a[c] += expf(tj - m[c]);
  }
#pragma unroll
  for (int c = 0; c < IPT; ++c) lse[c] = l.valid[c] ? m[c] + logf(a[c]) : 0.0f;
}

template <int G, bool BWD>
__global__ void __launch_bounds__(kLwThreads) listwise_pairsum_kernel(int kind, const float *__restrict__ labels,
                                                                      const float *__restrict__ scores, int64_t nlists,
                                                                      int len, int P, float alpha,
                                                                      const float *__restrict__ scale,
                                                                      float *__restrict__ out) {
  constexpr int IPT = LwCfg<G>::IPT;
  __shared__ LwShared<G> sh;
  LwList<G> l;
  lw_load<G>(l, sh, labels, scores, nlists, len);
  const int64_t list = (int64_t)blockIdx.x * LwCfg<G>::LPB + threadIdx.x / G;
  const float sc = (BWD && l.active) ? scale[list] : 0.0f;
  float g[IPT];        // BWD: gradient of the item a thread owns, before alpha
  float loss = 0.0f;   // !BWD: the list's loss
  bool live = true;    // the list has a loss (approx kinds: IDCG, Y > 0)

  if (kind == kPsUniqueSoftmax) {
    float *t = sh.m[1] + l.off, *lsej = sh.m[0] + l.off, *gainj = sh.a[0] + l.off;
#pragma unroll
    for (int c = 0; c < IPT; ++c) t[l.sub + G * c] = alpha * l.sv[c];
    __syncthreads();
    float ti[IPT], lse[IPT], gain[IPT];
    lw_unique_lse<G>(l, sh, len, t, ti, lse);
#pragma unroll
    for (int c = 0; c < IPT; ++c) gain[c] = l.valid[c] ? exp2f(l.yv[c]) - 1.0f : 0.0f;
    if (!BWD) {
      float v = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (l.valid[c]) v += gain[c] * (lse[c] - ti[c]);
      loss = lw_sum<G>(v, sh.red);
    } else {
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        lsej[l.sub + G * c] = lse[c];
        gainj[l.sub + G * c] = gain[c];
        g[c] = 0.0f;
      }
      __syncthreads();
      for (int j = 0; j < len; ++j) {
        const float yj = sh.y[l.off + j], lj = lsej[j], gj = gainj[j];
        if (!(yj >= 0.0f)) continue;
#pragma unroll
        for (int c = 0; c < IPT; ++c) {
          if (!l.valid[c]) continue;
          if (l.sub + G * c == j) g[c] += gj * (expf(ti[c] - lj) - 1.0f);
          else if (yj > l.yv[c]) g[c] += gj * expf(ti[c] - lj);
        }
      }
    }
  } else {             // ApproxNDCG, ApproxMRR
    float norm;        // IDCG, or Y
    if (kind == kPsApproxNdcg) {
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int i = l.sub + G * c;
        sh.key[l.off + i] = l.valid[c] ? make_key(l.yv[c], i) : 0ull;
      }
      __syncthreads();
      lw_sort<G>(l, sh, P);
      float v = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        const int r = l.sub + G * c;
        const uint64_t k = r < P ? sh.key[l.off + r] : 0ull;
        if (k != 0ull) v += (exp2f(sh.y[l.off + key_index(k)]) - 1.0f) / log2f((float)(r + 2));
      }
      norm = lw_sum<G>(v, sh.red);
    } else {
      float v = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) if (l.valid[c]) v += l.yv[c];
      norm = lw_sum<G>(v, sh.red);
    }
    live = norm > 0.0f;
    float r[IPT];
    lw_soft_ranks<G>(l, sh, len, alpha, r);
    if (!BWD) {
      float v = 0.0f;
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        if (!l.valid[c]) continue;
        if (kind == kPsApproxNdcg) v += (exp2f(l.yv[c]) - 1.0f) / log2f(1.0f + r[c]);
        else v += l.yv[c] / r[c];
      }
      v = lw_sum<G>(v, sh.red);
      loss = live ? -(v / norm) : 0.0f;
    } else {
      float *cj = sh.m[0] + l.off;
      float ck[IPT];
#pragma unroll
      for (int c = 0; c < IPT; ++c) {
        ck[c] = 0.0f;
        if (l.valid[c] && live) {
          if (kind == kPsApproxNdcg) {
            const float lg = log2f(1.0f + r[c]);
            ck[c] = (exp2f(l.yv[c]) - 1.0f) / (((norm * kLwLn2) * (1.0f + r[c])) * (lg * lg));
          } else {
            ck[c] = l.yv[c] / ((norm * r[c]) * r[c]);
          }
        }
        cj[l.sub + G * c] = ck[c];
        g[c] = 0.0f;
      }
      __syncthreads();
      for (int j = 0; j < len; ++j) {
        const float yj = sh.y[l.off + j], sj = sh.s[l.off + j], c_j = cj[j];
        if (!(yj >= 0.0f)) continue;
#pragma unroll
        for (int c = 0; c < IPT; ++c)
          if (l.valid[c] && l.sub + G * c != j) g[c] += (c_j - ck[c]) * lw_sigmoid_grad(alpha * (l.sv[c] - sj));
      }
    }
  }

  if (BWD) {
#pragma unroll
    for (int c = 0; c < IPT; ++c) {
      const int i = l.sub + G * c;
      if (l.active && i < len) out[l.base + i] = (l.valid[c] && live) ? sc * (alpha * g[c]) : 0.0f;
    }
  } else if (l.active && l.sub == 0) {
    out[list] = loss;
  }
}

static int lw_group(int len) { return len <= 8 ? 8 : len <= 16 ? 16 : len <= 32 ? 32 : len <= 64 ? 64 : 256; }
static int lw_pow2(int len, int g) {
  int p = g < 256 ? g : 128;
  while (p < len) p <<= 1;
  return p;
}

static int lw_check_shape(const char *what, int64_t nlists, int len) {
  TFRS_CHECK_ARG(nlists >= 0, "%s: nlists must be non-negative", what);
  TFRS_CHECK_ARG(len >= 1 && len <= kLwMaxLen, "%s: len=%d outside 1 .. %d", what, len, kLwMaxLen);
  TFRS_CHECK_ARG(nlists * (int64_t)len < (1ll << 31), "%s: nlists * len must stay below 2^31", what);
  return TFRS_OK;
}

#define TFRS_LW_DISPATCH(KERNEL, ...)                                                                       \
  do {                                                                                                      \
    const int g_ = lw_group(len);                                                                           \
    const int P = lw_pow2(len, g_);                                                                         \
    const unsigned grid_ = (unsigned)((nlists + (kLwThreads / g_) - 1) / (kLwThreads / g_));                \
    switch (g_) {                                                                                           \
      case 8: hipLaunchKernelGGL((KERNEL(8)), dim3(grid_), dim3(kLwThreads), 0, s, __VA_ARGS__); break;     \
      case 16: hipLaunchKernelGGL((KERNEL(16)), dim3(grid_), dim3(kLwThreads), 0, s, __VA_ARGS__); break;   \
      case 32: hipLaunchKernelGGL((KERNEL(32)), dim3(grid_), dim3(kLwThreads), 0, s, __VA_ARGS__); break;   \
      case 64: hipLaunchKernelGGL((KERNEL(64)), dim3(grid_), dim3(kLwThreads), 0, s, __VA_ARGS__); break;   \
      default: hipLaunchKernelGGL((KERNEL(256)), dim3(grid_), dim3(kLwThreads), 0, s, __VA_ARGS__); break;  \
    }                                                                                                       \
  } while (0)

#define TFRS_LW_FWD(G) listwise_loss_kernel<G, false>
#define TFRS_LW_BWD(G) listwise_loss_kernel<G, true>
#define TFRS_LW_METRICS(G) listwise_metrics_kernel<G>
#define TFRS_LW_LAMBDA_FWD(G) listwise_lambda_kernel<G, false, false>
#define TFRS_LW_LAMBDA_FWD_SMOOTH(G) listwise_lambda_kernel<G, false, true>
#define TFRS_LW_LAMBDA_BWD(G) listwise_lambda_kernel<G, true, false>
#define TFRS_LW_LAMBDA_BWD_SMOOTH(G) listwise_lambda_kernel<G, true, true>
#define TFRS_LW_PAIRSUM_FWD(G) listwise_pairsum_kernel<G, false>
#define TFRS_LW_PAIRSUM_BWD(G) listwise_pairsum_kernel<G, true>

static int lw_check_lambda(const char *what, int kind, int topn, float smooth_fraction) {
  TFRS_CHECK_ARG(kind == kLwPairLogistic || kind == kLwPairHinge,
                 "%s: kind %d takes no lambda weight (pairwise logistic and pairwise hinge do)", what, kind);
  TFRS_CHECK_ARG(topn >= 0, "%s: topn=%d must be positive, or 0 for no cut", what, topn);
  TFRS_CHECK_ARG(smooth_fraction >= 0.0f && smooth_fraction <= 1.0f, "%s: smooth_fraction=%g outside [0, 1]", what,
                 (double)smooth_fraction);
  return TFRS_OK;
}

// temperature finite and positive with a finite float32 reciprocal: alpha = 1 / temperature is what the kernels take.
static int lw_check_pairsum(const char *what, int kind, float temperature) {
  TFRS_CHECK_ARG(kind >= kPsApproxNdcg && kind <= kPsUniqueSoftmax, "%s: unknown kind %d", what, kind);
  TFRS_CHECK_ARG(temperature > 0.0f && temperature <= 3.402823466e38f && 1.0f / temperature <= 3.402823466e38f,
                 "%s: temperature=%g must be finite and positive, with a finite float32 reciprocal", what,
                 (double)temperature);
  return TFRS_OK;
}

// One launch for validated arguments: the descriptor is built here, on the host, and travels as a kernel argument.
static int lw_launch_metrics(const float *labels, const float *scores, int64_t nlists, int len, int nmetrics,
                             const int *kinds, const int *topns, float *values, float *weights, hipStream_t s) {
  LwMetricDesc d = {};
  d.n = nmetrics;
  for (int m = 0; m < nmetrics; ++m) {
    const int k = kinds[m];
    d.kind[m] = k;
    d.topn[m] = topns[m];
    if (k != kLmOpa) {
      d.flags |= kLmScoreSort;
      const int cut = topns[m] > 0 ? topns[m] : kLwMaxLen;
      d.rank_lim = cut > d.rank_lim ? cut : d.rank_lim;
    }
    if (k == kLmNdcg) d.flags |= kLmLabelSort;
    if (k == kLmNdcg || k == kLmDcg) {
      d.flags |= kLmGain;
      const int cut = topns[m] > 0 ? topns[m] : kLwMaxLen;
      d.gain_lim = cut > d.gain_lim ? cut : d.gain_lim;
    }
    if (k == kLmDcg) d.flags |= kLmPositive;
    if (k == kLmMrr || k == kLmHits || k == kLmPrecision || k == kLmRecall || k == kLmMap) d.flags |= kLmCount;
    if (k == kLmArp) d.flags |= kLmArpSums;
    if (k == kLmOpa) d.flags |= kLmPairs;
  }
  TFRS_LW_DISPATCH(TFRS_LW_METRICS, labels, scores, values, weights, nlists, len, P, d);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

}  // namespace tfrs

using namespace tfrs;

extern "C" int tfrs_listwise_loss_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                      float *loss, void *stream) {
  TFRS_CHECK_ARG(kind >= kLwSoftmax && kind <= kLwListMle, "listwise_loss_fwd: unknown kind %d", kind);
  if (int rc = lw_check_shape("listwise_loss_fwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && loss, "listwise_loss_fwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const float *no_scale = nullptr;
  TFRS_LW_DISPATCH(TFRS_LW_FWD, kind, labels, scores, nlists, len, P, no_scale, loss);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_listwise_loss_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                      const float *scale, float *dscores, void *stream) {
  TFRS_CHECK_ARG(kind >= kLwSoftmax && kind <= kLwListMle, "listwise_loss_bwd: unknown kind %d", kind);
  if (int rc = lw_check_shape("listwise_loss_bwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && scale && dscores, "listwise_loss_bwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  TFRS_LW_DISPATCH(TFRS_LW_BWD, kind, labels, scores, nlists, len, P, scale, dscores);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_listwise_ndcg(const float *labels, const float *scores, int64_t nlists, int len, int topn,
                                  float *ndcg, float *counted, void *stream) {
  TFRS_CHECK_ARG(topn >= 0, "listwise_ndcg: topn=%d must be positive, or 0 for no cut", topn);
  if (int rc = lw_check_shape("listwise_ndcg", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && ndcg && counted, "listwise_ndcg: NULL pointer");
  const int kind = kLmNdcg;            // the one-metric call of the metrics kernel: values = ndcg, weights = counted
  return lw_launch_metrics(labels, scores, nlists, len, 1, &kind, &topn, ndcg, counted, (hipStream_t)stream);
}

extern "C" int tfrs_listwise_metrics(const float *labels, const float *scores, int64_t nlists, int len, int nmetrics,
                                     const int *kinds, const int *topns, float *values, float *weights, void *stream) {
  TFRS_CHECK_ARG(nmetrics >= 1 && nmetrics <= TFRS_LISTWISE_METRIC_MAX, "listwise_metrics: nmetrics=%d outside 1 .. %d",
                 nmetrics, TFRS_LISTWISE_METRIC_MAX);
  TFRS_CHECK_ARG(kinds && topns, "listwise_metrics: NULL kinds / topns array");
  for (int m = 0; m < nmetrics; ++m) {
    TFRS_CHECK_ARG(kinds[m] >= kLmNdcg && kinds[m] <= kLmOpa, "listwise_metrics: unknown kind %d (metric %d)", kinds[m], m);
    TFRS_CHECK_ARG(topns[m] >= 0, "listwise_metrics: topn=%d must be positive, or 0 for no cut (metric %d)", topns[m], m);
    TFRS_CHECK_ARG(topns[m] == 0 || (kinds[m] != kLmArp && kinds[m] != kLmOpa),
                   "listwise_metrics: ARP and OPA take no topn, got %d (metric %d)", topns[m], m);
  }
  if (int rc = lw_check_shape("listwise_metrics", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && values && weights, "listwise_metrics: NULL pointer");
  return lw_launch_metrics(labels, scores, nlists, len, nmetrics, kinds, topns, values, weights, (hipStream_t)stream);
}

extern "C" int tfrs_listwise_lambda_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                        int topn, int normalized, float smooth_fraction, float *loss, void *stream) {
  if (int rc = lw_check_lambda("listwise_lambda_fwd", kind, topn, smooth_fraction)) return rc;
  if (int rc = lw_check_shape("listwise_lambda_fwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && loss, "listwise_lambda_fwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const float *no_scale = nullptr;
  if (smooth_fraction != 0.0f)
    TFRS_LW_DISPATCH(TFRS_LW_LAMBDA_FWD_SMOOTH, kind, labels, scores, nlists, len, P, topn, normalized, smooth_fraction,
                     no_scale, loss);
  else
    TFRS_LW_DISPATCH(TFRS_LW_LAMBDA_FWD, kind, labels, scores, nlists, len, P, topn, normalized, smooth_fraction,
                     no_scale, loss);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_listwise_lambda_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                        int topn, int normalized, float smooth_fraction, const float *scale,
                                        float *dscores, void *stream) {
  if (int rc = lw_check_lambda("listwise_lambda_bwd", kind, topn, smooth_fraction)) return rc;
  if (int rc = lw_check_shape("listwise_lambda_bwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && scale && dscores, "listwise_lambda_bwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (smooth_fraction != 0.0f)
    TFRS_LW_DISPATCH(TFRS_LW_LAMBDA_BWD_SMOOTH, kind, labels, scores, nlists, len, P, topn, normalized, smooth_fraction,
                     scale, dscores);
  else
    TFRS_LW_DISPATCH(TFRS_LW_LAMBDA_BWD, kind, labels, scores, nlists, len, P, topn, normalized, smooth_fraction, scale,
                     dscores);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_listwise_pairsum_fwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                         float temperature, float *loss, void *stream) {
  if (int rc = lw_check_pairsum("listwise_pairsum_fwd", kind, temperature)) return rc;
  if (int rc = lw_check_shape("listwise_pairsum_fwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && loss, "listwise_pairsum_fwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const float alpha = 1.0f / temperature;
  const float *no_scale = nullptr;
  TFRS_LW_DISPATCH(TFRS_LW_PAIRSUM_FWD, kind, labels, scores, nlists, len, P, alpha, no_scale, loss);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_listwise_pairsum_bwd(int kind, const float *labels, const float *scores, int64_t nlists, int len,
                                         float temperature, const float *scale, float *dscores, void *stream) {
  if (int rc = lw_check_pairsum("listwise_pairsum_bwd", kind, temperature)) return rc;
  if (int rc = lw_check_shape("listwise_pairsum_bwd", nlists, len)) return rc;
  if (nlists == 0) return TFRS_OK;
  TFRS_CHECK_ARG(labels && scores && scale && dscores, "listwise_pairsum_bwd: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const float alpha = 1.0f / temperature;
  TFRS_LW_DISPATCH(TFRS_LW_PAIRSUM_BWD, kind, labels, scores, nlists, len, P, alpha, scale, dscores);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
