// numeric.hip -- the numeric preprocessing layers: Discretization (bucketize) and Normalization (normalize, moments).
//
// Replaces tf.keras.layers.Discretization / Normalization, which the reference's tutorials put on the timestamp
// feature of the user tower.  Three families of kernels, all memory-bound, one read and one write per
// element (the moments read only):
//
//   bucketize   out[i] = #{ j : !(x[i] < b[j]) } -- std::upper_bound, what TensorFlow's Bucketize kernel runs.  The
//               boundaries are f32 (the op's attribute is a list of 32-bit floats): f32 / int32 / int64 input is
//               compared in f32 (integers converted with round-to-nearest-even), f64 input in f64 against the
//               widened boundaries.  NaN compares false with everything and lands in bucket nb.
//   normalize   (x - mean) / scale in f32 (an IEEE subtraction, then an IEEE division), its inverse
//               fma(x, scale, mean), and the backward of either.
//   moments     per feature (count, mean, M2) in f64 of the f32-converted values: every workgroup reduces a slice of
//               rows to one partial per feature, a second launch of ONE workgroup merges the partials into the running
//               state with Chan's pairwise update, in an order fixed by the shape alone -- no atomics, the same bits on
//               every run.
//
// The search is branch-free: the boundaries are padded with +inf to P - 1 entries, P the power of two above nb, and
// log2(P) steps of `pos += step` under a compare walk it; every lane of a wave runs the same number of steps.  Up to
// TFRS_BUCKETIZE_LDS_BOUNDARIES boundaries a workgroup stages the padded list in LDS once and every probe is a
// ds_read_b32; beyond, the probes go to global memory (the list is L2-resident) with the pad applied by index.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace tfrs {

constexpr int kNumericMaxBlocks = 2048;   // grid cap of the element-wise kernels: grid-stride beyond
constexpr int kVectorsPerLane = 4;        // 16-byte loads a lane issues before the grid grows

template <typename T> struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };
struct alignas(16) I64x2 { int64_t a, b; };

// ---- what one 16-byte-aligned walk over n elements looks like: a scalar head up to the first aligned address, whole
// vectors, a scalar tail --------------------------------------------------------------------------------------------
struct Walk {
  int64_t head, nvec, tail_at, n;
};
template <typename T> static inline Walk make_walk(const void *x, int64_t n) {
  constexpr int64_t V = 16 / sizeof(T);
  Walk w;
  const int64_t to_aligned = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(T));
  w.head = std::min<int64_t>(to_aligned, n);
  w.nvec = (n - w.head) / V;
  w.tail_at = w.head + w.nvec * V;
  w.n = n;
  return w;
}
static inline unsigned walk_grid(const Walk &w) {
  const int64_t per_block = 256 * (int64_t)kVectorsPerLane;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((w.nvec + per_block - 1) / per_block, kNumericMaxBlocks));
}

// ---- bucketize -----------------------------------------------------------------------------------------------------
template <typename T> struct CompareAs { using type = float; };     // f32 / int32 / int64: compared in f32 (RNE)
template <> struct CompareAs<double> { using type = double; };      // f64: against the widened boundaries

// LDS: b[0 .. P - 2] holds the boundaries, +inf from nb on.  pos never exceeds P - 1 >= nb; +inf (every pad counts) and
// NaN (every entry counts) are cut back to nb.
template <typename C> __device__ __forceinline__ int64_t search_lds(const float *b, int p, int nb, C x) {
  int pos = 0;
#pragma unroll 1
  for (int step = p >> 1; step >= 1; step >>= 1) pos += (x < (C)b[pos + step - 1]) ? 0 : step;
  return (int64_t)(pos < nb ? pos : nb);
}
template <typename C>
__device__ __forceinline__ int64_t search_global(const float *__restrict__ b, int64_t p, int64_t nb, C x) {
  int64_t pos = 0;
#pragma unroll 1
  for (int64_t step = p >> 1; step >= 1; step >>= 1) {
    const int64_t at = pos + step - 1;
    const bool below = at < nb ? (x < (C)b[at]) : (x < (C)INFINITY);
    pos += below ? 0 : step;
  }
  return pos < nb ? pos : nb;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(256) bucketize_kernel(const T *__restrict__ x, Walk w,
                                                        const float *__restrict__ boundaries, int64_t nb, int64_t p,
                                                        int64_t *__restrict__ out) {
  using C = typename CompareAs<T>::type;
  constexpr int V = 16 / sizeof(T);
  extern __shared__ __align__(16) float lds_b[];
  if (LDS) {
    for (int j = threadIdx.x; j < (int)p - 1; j += 256) lds_b[j] = j < nb ? boundaries[j] : INFINITY;
    __syncthreads();
  }
  auto find = [&](T value) -> int64_t {
    const C c = (C)value;
    return LDS ? search_lds<C>(lds_b, (int)p, (int)nb, c) : search_global<C>(boundaries, p, nb, c);
  };
  // head and tail: at most V - 1 elements each, taken by the first lanes of workgroup 0
  if (blockIdx.x == 0) {
    const int64_t edge = w.head + (w.n - w.tail_at);
    if (threadIdx.x < edge) {
      const int64_t e = threadIdx.x < w.head ? threadIdx.x : w.tail_at + (threadIdx.x - w.head);
      out[e] = find(x[e]);
    }
  }
  const Vec16<T> *__restrict__ xv = reinterpret_cast<const Vec16<T> *>(x + w.head);
  int64_t *__restrict__ ov = out + w.head;
  const bool out_aligned = (((uintptr_t)ov) & 15) == 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < w.nvec; v += (int64_t)gridDim.x * 256) {
    const Vec16<T> in = xv[v];
    int64_t r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = find(in.v[k]);
    if (out_aligned) {
#pragma unroll
      for (int k = 0; k < V; k += 2) {
        I64x2 pair;
        pair.a = r[k];
        pair.b = r[k + 1];
        *reinterpret_cast<I64x2 *>(ov + v * V + k) = pair;
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) ov[v * V + k] = r[k];
    }
  }
}

// ---- normalize -----------------------------------------------------------------------------------------------------
enum { kNormForward = 0, kNormInvert = 1, kNormBackward = 2, kNormBackwardInvert = 3 };

template <int MODE> __device__ __forceinline__ float normalize_one(float x, float mean, float scale) {
  if (MODE == kNormForward) return (x - mean) / scale;      // two IEEE operations, never contracted
  if (MODE == kNormInvert) return fmaf(x, scale, mean);
  if (MODE == kNormBackward) return x / scale;
  return x * scale;
}

// F1: one mean and one scale (axis=None).  Otherwise the feature of flat element e is e mod f.
template <typename T, int MODE, bool F1>
__global__ void __launch_bounds__(256) normalize_kernel(const T *__restrict__ x, Walk w, int64_t f,
                                                        const float *__restrict__ mean,
                                                        const float *__restrict__ scale, float *__restrict__ out) {
  constexpr int V = 16 / sizeof(T);
  const bool narrow = w.n <= 0xFFFFFFFFll;    // 32-bit remainder where the element index fits
  auto column = [&](int64_t e) -> int64_t {
    if (F1) return 0;
    return narrow ? (int64_t)((uint32_t)e % (uint32_t)f) : e % f;
  };
  const float m1 = mean[0], s1 = scale[0];
  if (blockIdx.x == 0) {
    const int64_t edge = w.head + (w.n - w.tail_at);
    if (threadIdx.x < edge) {
      const int64_t e = threadIdx.x < w.head ? threadIdx.x : w.tail_at + (threadIdx.x - w.head);
      const int64_t c = column(e);
      out[e] = normalize_one<MODE>((float)x[e], F1 ? m1 : mean[c], F1 ? s1 : scale[c]);
    }
  }
  const Vec16<T> *__restrict__ xv = reinterpret_cast<const Vec16<T> *>(x + w.head);
  float *__restrict__ ov = out + w.head;
  const bool out_aligned = (((uintptr_t)ov) & 15) == 0 && V == 4;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < w.nvec; v += (int64_t)gridDim.x * 256) {
    const Vec16<T> in = xv[v];
    int64_t c = column(w.head + v * V);
    float r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      r[k] = normalize_one<MODE>((float)in.v[k], F1 ? m1 : mean[c], F1 ? s1 : scale[c]);
      if (!F1) c = c + 1 == f ? 0 : c + 1;
    }
    if (out_aligned) {
      Vec16<float> o;
#pragma unroll
      for (int k = 0; k < V; ++k) o.v[k & 3] = r[k];
      *reinterpret_cast<Vec16<float> *>(ov + v * V) = o;
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) ov[v * V + k] = r[k];
    }
  }
}

// ---- moments -------------------------------------------------------------------------------------------------------
// A partial is (count, mean, M2 = sum of squared deviations from that mean), three doubles.
struct Moments {
  double n, mean, m2;
};

// Chan, Golub, LeVeque: the moments of the union of two disjoint samples.  An empty side leaves the other unchanged,
// bit for bit.
__device__ __forceinline__ Moments merge(const Moments &a, const Moments &b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Moments r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  const double wb = b.n / r.n;
  r.mean = a.mean + delta * wb;
  r.m2 = a.m2 + b.m2 + delta * delta * (a.n * wb);
  return r;
}

// Lane layout of one workgroup over a chunk of `width` <= 256 columns: `lanes_r` = 256 / width row lanes per column,
// lane t = r * width + c.  Small f keeps the wave busy: f = 1 uses 256 lanes, f = 3 255, f = 13 247.
// tree_merge folds the row lanes of each column in LDS, partner r + s for s = 128, 64, ... 1: an order fixed by
// (width, lanes_r) alone.  The result of column c is in lane c (r = 0).
__device__ __forceinline__ Moments tree_merge(Moments mine, double *lds, int width, int lanes_r, bool active, int r) {
  const int t = threadIdx.x;
  __syncthreads();        // the previous chunk's readers are done with lds
  if (active) {
    lds[3 * t + 0] = mine.n;
    lds[3 * t + 1] = mine.mean;
    lds[3 * t + 2] = mine.m2;
  }
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (active && r < s && r + s < lanes_r) {
      const int o = t + s * width;
      Moments other;
      other.n = lds[3 * o + 0];
      other.mean = lds[3 * o + 1];
      other.m2 = lds[3 * o + 2];
      mine = merge(mine, other);
      lds[3 * t + 0] = mine.n;
      lds[3 * t + 1] = mine.mean;
      lds[3 * t + 2] = mine.m2;
    }
    __syncthreads();
  }
  return mine;
}

// Stage 1.  Workgroup g owns rows [g * slice_rows, min(n_rows, (g + 1) * slice_rows)).  A lane sums its column's values
// shifted by the first one it meets, K: with d = x - K (exact in f64 for f32 values of like magnitude)
//   mean = K + sum(d) / n,   M2 = sum(d^2) - sum(d)^2 / n,
// which cancels only in proportion to ((K - mean) / sigma)^2 and K is itself a sample.  Constant data gives d = 0
// throughout, so M2 is exactly 0; rounding can make M2 negative by an ulp of sum(d^2), which is cut to 0 (NaN stays).
template <typename T>
__global__ void __launch_bounds__(256) moments_partial_kernel(const T *__restrict__ x, int64_t n_rows, int64_t f,
                                                              int64_t slice_rows, double *__restrict__ partials) {
  __shared__ double lds[256 * 3];
  const int t = threadIdx.x;
  const int64_t row_lo = (int64_t)blockIdx.x * slice_rows;
  const int64_t row_hi = row_lo + slice_rows < n_rows ? row_lo + slice_rows : n_rows;
  for (int64_t c0 = 0; c0 < f; c0 += 256) {
    const int width = (int)(f - c0 < 256 ? f - c0 : 256);
    const int lanes_r = 256 / width;
    const bool active = t < lanes_r * width;
    const int r = t / width, c = t - r * width;
    Moments mine = {0.0, 0.0, 0.0};
    if (active) {
      double k = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
      const T *__restrict__ col = x + c0 + c;
      for (int64_t row = row_lo + r; row < row_hi; row += lanes_r) {
        const double v = (double)(float)col[row * f];
        if (cnt == 0.0) k = v;
        const double d = v - k;
        s1 += d;
        s2 = fma(d, d, s2);
        cnt += 1.0;
      }
      if (cnt > 0.0) {
        const double m2 = s2 - s1 * (s1 / cnt);
        mine.n = cnt;
        mine.mean = k + s1 / cnt;
        mine.m2 = m2 < 0.0 ? 0.0 : m2;
      }
    }
    mine = tree_merge(mine, lds, width, lanes_r, active, r);
    if (active && r == 0) {
      double *p = partials + ((int64_t)blockIdx.x * f + c0 + c) * 3;
      p[0] = mine.n;
      p[1] = mine.mean;
      p[2] = mine.m2;
    }
  }
}

// Stage 2, ONE workgroup: row lane r of column c folds partials r, r + lanes_r, ... in that order, the tree folds the
// row lanes, and lane r = 0 merges the batch into state[c].
__global__ void __launch_bounds__(256) moments_merge_kernel(const double *__restrict__ partials, int64_t groups,
                                                            int64_t f, double *__restrict__ state) {
  __shared__ double lds[256 * 3];
  const int t = threadIdx.x;
  for (int64_t c0 = 0; c0 < f; c0 += 256) {
    const int width = (int)(f - c0 < 256 ? f - c0 : 256);
    const int lanes_r = 256 / width;
    const bool active = t < lanes_r * width;
    const int r = t / width, c = t - r * width;
    Moments mine = {0.0, 0.0, 0.0};
    if (active) {
      for (int64_t g = r; g < groups; g += lanes_r) {
        const double *p = partials + (g * f + c0 + c) * 3;
        Moments other = {p[0], p[1], p[2]};
        mine = merge(mine, other);
      }
    }
    mine = tree_merge(mine, lds, width, lanes_r, active, r);
    if (active && r == 0) {
      double *s = state + (c0 + c) * 3;
      Moments before = {s[0], s[1], s[2]};
      const Moments after = merge(before, mine);
      s[0] = after.n;
      s[1] = after.mean;
      s[2] = after.m2;
    }
  }
}

// mean and population variance rounded to f32 once; the square root of the f32 variance through f64, whose rounding
// to f32 is the correctly rounded f32 root (53 >= 2 * 24 + 2).  No data yet: Keras' reset values, mean 0, variance 1.
__global__ void __launch_bounds__(256) moments_finalize_kernel(const double *__restrict__ state, int64_t f,
                                                               float *__restrict__ mean, float *__restrict__ var,
                                                               float *__restrict__ scale) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < f; c += (int64_t)gridDim.x * 256) {
    const double n = state[3 * c];
    float m = 0.0f, v = 1.0f;
    if (n > 0.0) {
      m = (float)state[3 * c + 1];
      v = (float)(state[3 * c + 2] / n);
    }
    const float root = (float)sqrt((double)v);
    mean[c] = m;
    var[c] = v;
    scale[c] = root > TFRS_NORMALIZE_EPSILON ? root : (root != root ? root : TFRS_NORMALIZE_EPSILON);
  }
}

__global__ void __launch_bounds__(256) moments_reset_kernel(double *__restrict__ state, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) state[i] = 0.0;
}

}  // namespace tfrs

using namespace tfrs;

static inline int dtype_bytes(int dtype) {
  switch (dtype) {
    case TFRS_NUMERIC_F32: return 4;
    case TFRS_NUMERIC_F64: return 8;
    case TFRS_NUMERIC_I32: return 4;
    case TFRS_NUMERIC_I64: return 8;
    default: return 0;
  }
}

static inline int64_t pow2_above(int64_t nb) {   // the smallest power of two > nb
  int64_t p = 1;
  while (p <= nb) p <<= 1;
  return p;
}

template <typename T>
static int launch_bucketize(const void *x, int64_t n, const float *boundaries, int64_t nb, int64_t *out,
                            hipStream_t s) {
  const Walk w = make_walk<T>(x, n);
  const int64_t p = pow2_above(nb);
  if (nb <= TFRS_BUCKETIZE_LDS_BOUNDARIES)
    hipLaunchKernelGGL((bucketize_kernel<T, true>), dim3(walk_grid(w)), dim3(256), (size_t)p * sizeof(float), s,
                       (const T *)x, w, boundaries, nb, p, out);
  else
    hipLaunchKernelGGL((bucketize_kernel<T, false>), dim3(walk_grid(w)), dim3(256), 0, s, (const T *)x, w, boundaries,
                       nb, p, out);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_bucketize(const void *x, int dtype, int64_t n, const float *boundaries, int64_t nb, int64_t *out,
                              void *stream) {
  const int bytes = dtype_bytes(dtype);
  TFRS_CHECK_ARG(bytes, "bucketize: unknown dtype code %d", dtype);
  TFRS_CHECK_ARG(n >= 0 && nb >= 0 && nb < (1ll << 40), "bucketize: bad count (n %lld, nb %lld)", (long long)n,
                 (long long)nb);
  TFRS_CHECK_ARG(boundaries || nb == 0, "bucketize: NULL boundaries");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG(x && out, "bucketize: NULL pointer");
  TFRS_CHECK_ARG(((uintptr_t)x) % bytes == 0 && ((uintptr_t)out) % 8 == 0, "bucketize: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case TFRS_NUMERIC_F32: return launch_bucketize<float>(x, n, boundaries, nb, out, s);
    case TFRS_NUMERIC_F64: return launch_bucketize<double>(x, n, boundaries, nb, out, s);
    case TFRS_NUMERIC_I32: return launch_bucketize<int32_t>(x, n, boundaries, nb, out, s);
    default: return launch_bucketize<int64_t>(x, n, boundaries, nb, out, s);
  }
}

template <typename T, int MODE>
static int launch_normalize_mode(const void *x, int64_t n, int64_t f, const float *mean, const float *scale,
                                 float *out, hipStream_t s) {
  const Walk w = make_walk<T>(x, n);
  if (f == 1)
    hipLaunchKernelGGL((normalize_kernel<T, MODE, true>), dim3(walk_grid(w)), dim3(256), 0, s, (const T *)x, w, f,
                       mean, scale, out);
  else
    hipLaunchKernelGGL((normalize_kernel<T, MODE, false>), dim3(walk_grid(w)), dim3(256), 0, s, (const T *)x, w, f,
                       mean, scale, out);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

template <typename T>
static int launch_normalize(const void *x, int64_t n, int64_t f, const float *mean, const float *scale, int mode,
                            float *out, hipStream_t s) {
  switch (mode) {
    case kNormForward: return launch_normalize_mode<T, kNormForward>(x, n, f, mean, scale, out, s);
    case kNormInvert: return launch_normalize_mode<T, kNormInvert>(x, n, f, mean, scale, out, s);
    case kNormBackward: return launch_normalize_mode<T, kNormBackward>(x, n, f, mean, scale, out, s);
    default: return launch_normalize_mode<T, kNormBackwardInvert>(x, n, f, mean, scale, out, s);
  }
}

extern "C" int tfrs_normalize(const void *x, int dtype, int64_t n_rows, int64_t f, const float *mean,
                              const float *scale, int mode, float *out, void *stream) {
  const int bytes = dtype_bytes(dtype);
  TFRS_CHECK_ARG(bytes, "normalize: unknown dtype code %d", dtype);
  TFRS_CHECK_ARG(mode >= 0 && mode <= 3, "normalize: unknown mode %d", mode);
  TFRS_CHECK_ARG(n_rows >= 0 && f >= 1 && f < (1ll << 31) && n_rows <= INT64_MAX / f,
                 "normalize: bad shape (n_rows %lld, f %lld)", (long long)n_rows, (long long)f);
  TFRS_CHECK_ARG(mean && scale, "normalize: NULL statistics");
  if (n_rows == 0) return TFRS_OK;
  TFRS_CHECK_ARG(x && out, "normalize: NULL pointer");
  TFRS_CHECK_ARG(((uintptr_t)x) % bytes == 0 && ((uintptr_t)out) % 4 == 0, "normalize: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = n_rows * f;
  switch (dtype) {
    case TFRS_NUMERIC_F32: return launch_normalize<float>(x, n, f, mean, scale, mode, out, s);
    case TFRS_NUMERIC_F64: return launch_normalize<double>(x, n, f, mean, scale, mode, out, s);
    case TFRS_NUMERIC_I32: return launch_normalize<int32_t>(x, n, f, mean, scale, mode, out, s);
    default: return launch_normalize<int64_t>(x, n, f, mean, scale, mode, out, s);
  }
}

// rows per stage-1 workgroup: TFRS_MOMENTS_SLICE_ELEMENTS elements' worth, more once TFRS_MOMENTS_MAX_GROUPS slices
// no longer cover the batch
static inline int64_t moments_slice_rows(int64_t n_rows, int64_t f) {
  const int64_t base = std::max<int64_t>(1, (TFRS_MOMENTS_SLICE_ELEMENTS + f - 1) / f);
  return std::max<int64_t>(base, (n_rows + TFRS_MOMENTS_MAX_GROUPS - 1) / TFRS_MOMENTS_MAX_GROUPS);
}

extern "C" size_t tfrs_moments_workspace_bytes(int64_t n_rows, int64_t f) {
  if (n_rows < 0 || f < 1) return 0;
  // an upper bound of the slices of every batch of at most n_rows rows, so that it never decreases in n_rows
  const int64_t base = std::max<int64_t>(1, (TFRS_MOMENTS_SLICE_ELEMENTS + f - 1) / f);
  const int64_t groups = std::max<int64_t>(1, std::min<int64_t>((n_rows + base - 1) / base, TFRS_MOMENTS_MAX_GROUPS));
  return (size_t)groups * (size_t)f * 3 * sizeof(double);
}

extern "C" int tfrs_moments_update(const void *x, int dtype, int64_t n_rows, int64_t f, double *state, void *workspace,
                                   size_t workspace_bytes, void *stream) {
  const int bytes = dtype_bytes(dtype);
  TFRS_CHECK_ARG(bytes, "moments_update: unknown dtype code %d", dtype);
  TFRS_CHECK_ARG(n_rows >= 0 && f >= 1 && f < (1ll << 31) && n_rows <= INT64_MAX / f,
                 "moments_update: bad shape (n_rows %lld, f %lld)", (long long)n_rows, (long long)f);
  TFRS_CHECK_ARG(state && ((uintptr_t)state) % 8 == 0, "moments_update: state must be non-NULL and 8-byte aligned");
  if (n_rows == 0) return TFRS_OK;
  const int64_t slice_rows = moments_slice_rows(n_rows, f);
  const int64_t groups = (n_rows + slice_rows - 1) / slice_rows;
  TFRS_CHECK_ARG(x && workspace, "moments_update: NULL pointer");
  TFRS_CHECK_ARG(((uintptr_t)x) % bytes == 0 && ((uintptr_t)workspace) % 8 == 0, "moments_update: misaligned pointer");
  TFRS_CHECK_ARG(workspace_bytes >= (size_t)groups * (size_t)f * 3 * sizeof(double),
                 "moments_update: workspace of %zu bytes, %zu needed", workspace_bytes,
                 (size_t)groups * (size_t)f * 3 * sizeof(double));
  hipStream_t s = (hipStream_t)stream;
  double *partials = (double *)workspace;
  const dim3 grid((unsigned)groups), block(256);
  switch (dtype) {
    case TFRS_NUMERIC_F32:
      hipLaunchKernelGGL(moments_partial_kernel<float>, grid, block, 0, s, (const float *)x, n_rows, f, slice_rows,
                         partials);
      break;
    case TFRS_NUMERIC_F64:
      hipLaunchKernelGGL(moments_partial_kernel<double>, grid, block, 0, s, (const double *)x, n_rows, f, slice_rows,
                         partials);
      break;
    case TFRS_NUMERIC_I32:
      hipLaunchKernelGGL(moments_partial_kernel<int32_t>, grid, block, 0, s, (const int32_t *)x, n_rows, f,
                         slice_rows, partials);
      break;
    default:
      hipLaunchKernelGGL(moments_partial_kernel<int64_t>, grid, block, 0, s, (const int64_t *)x, n_rows, f,
                         slice_rows, partials);
      break;
  }
  TFRS_LAUNCH_CHECK();
  hipLaunchKernelGGL(moments_merge_kernel, dim3(1), block, 0, s, (const double *)partials, groups, f, state);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_moments_finalize(const double *state, int64_t f, float *mean, float *variance, float *scale,
                                     void *stream) {
  TFRS_CHECK_ARG(f >= 1 && f < (1ll << 31), "moments_finalize: bad feature count %lld", (long long)f);
  TFRS_CHECK_ARG(state && mean && variance && scale, "moments_finalize: NULL pointer");
  const unsigned grid = (unsigned)std::min<int64_t>((f + 255) / 256, kNumericMaxBlocks);
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, state, f, mean, variance,
                     scale);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_moments_reset(double *state, int64_t f, void *stream) {
  TFRS_CHECK_ARG(f >= 1 && f < (1ll << 31), "moments_reset: bad feature count %lld", (long long)f);
  TFRS_CHECK_ARG(state, "moments_reset: NULL pointer");
  const unsigned grid = (unsigned)std::min<int64_t>((3 * f + 255) / 256, kNumericMaxBlocks);
  hipLaunchKernelGGL(moments_reset_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, state, 3 * f);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
