// text.hip -- TextVectorization: standardise, split and look up packed strings in one launch.
//
// Replaces the tf.keras.layers.TextVectorization layer in front of the title tower of the reference's retrieval
// tutorials: bytes in HBM -> token indices, without the host.  The rules are byte rules, ASCII only:
//   lower              A-Z -> a-z
//   strip punctuation  the 32 bytes !"#$%&'()*+,-./:;<=>?@[\]^_`{|}~ are DELETED (it's -> its, a-b -> ab)
//   split whitespace   tokens are maximal runs of bytes other than space \t \n \v \f \r; a run whose bytes were all
//                      deleted is no token.  Without a split the standardised string is one token (none when empty).
// Bytes 0x80-0xFF pass unchanged.
//
// ONE tokeniser body (text_kernel) with a functor for what happens to a finished token:
//   CountEmit   counts[i] = tokens of string i
//   LookupEmit  SipHash-2-4 fingerprint of the standardised bytes (siphash.h, the key of tfrs_fingerprint_bytes) ->
//               table probe (vocab_probe.h, the probe of tfrs_vocab_lookup) -> 2 + value, or 1 when unknown; dense
//               [n, seq_len] rows zero-filled past the last token, or ragged at row_splits
//   SpanEmit    the fingerprint and the span [start, end) of the token's RAW bytes (adapt)
//
// Integer work, latency-bound like the lookup it ends in.  One lane owns one string and carries its state across
// the string: the SipHash state, the partly filled 64-bit word, the filtered token length and the token count.  A
// kept byte is shifted into the word, every eighth byte is absorbed, and whitespace or the string's end finishes a
// token of non-zero filtered length -- deleted punctuation never needs a compaction pass.  The byte loop is nested
// (Tokeniser::consume): the inner loop ends with a run, so the lanes of a wave finalise and probe their tokens
// together.  ONE very long string is walked by one lane: correct, and slow for that string alone.
//
// Two ways to the bytes (template flag WINDOW; the choice follows profiles/text_vectorization.jsonl -- the window
// while a workgroup's span fits one window on average, else the direct read -- and TFRS_TEXT_VARIANT forces one):
//   direct  each lane reads its own bytes from global memory
//   window  the 256 strings of a workgroup are consecutive in the blob: the workgroup streams its byte span
//           offsets[first] .. offsets[last + 1] through an LDS window of TFRS_TEXT_WINDOW_BYTES with coalesced
//           16-byte loads, and between two barriers every lane consumes the bytes of its string that fall inside
//           the window.  The number of windows comes from the workgroup-uniform span, so every lane reaches every
//           barrier.
//
// TWO robustness rules:
//   The kernel never reads outside [0, n_bytes), whatever the alignment of the blob pointer or of a span's ends:
//   a 16-byte piece of a window that is not wholly inside the blob is loaded bytewise under a guard.
//   Every lane clamps its offsets[i] and offsets[i + 1] into [0, n_bytes] and to lo <= hi (the workgroup clamps its
//   span the same way): malformed offsets give wrong indices, never a read out of bounds.
#include "common.h"
#include "siphash.h"
#include "vocab_probe.h"

namespace tfrs {

constexpr int kTextWindow = TFRS_TEXT_WINDOW_BYTES;
constexpr int kTextMaxBlocks = TFRS_TEXT_MAX_BLOCKS;   // grid cap, grid-stride beyond (as in vocab.hip)

__device__ __forceinline__ bool text_is_space(uint32_t c) { return c == 32u || c - 9u <= 4u; }   // \t \n \v \f \r
__device__ __forceinline__ bool text_is_punct(uint32_t c) {
  return c - 33u <= 14u || c - 58u <= 6u || c - 91u <= 5u || c - 123u <= 3u;
}
__device__ __forceinline__ int64_t text_clamp(int64_t x, int64_t lo, int64_t hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// The state a lane carries across its string.
template <typename Emit>
struct Tokeniser {
  Sip sip;
  uint64_t word;      // kept bytes of the token not yet absorbed, little-endian
  int64_t flen;       // kept bytes of the token so far
  int64_t count;      // finished tokens of the string
  int64_t start;      // where the token's run of raw bytes began

  __device__ __forceinline__ explicit Tokeniser(int64_t lo)
      : sip(kFingerprintK0, kFingerprintK1), word(0), flen(0), count(0), start(lo) {}

  __device__ __forceinline__ void finish(int64_t end, const Emit &emit, const typename Emit::Row &row) {
    if (flen > 0) {
      sip.absorb(word | ((uint64_t)(flen & 0xff) << 56));
      emit.token(row, count, sip.finish(), start, end);
      ++count;
      sip = Sip(kFingerprintK0, kFingerprintK1);
      word = 0;
      flen = 0;
    }
  }

  // One byte of the string; true when it ended a run of token bytes (whitespace under the split).
  __device__ __forceinline__ bool feed(uint32_t c, int standardize, int split) {
    if (split && text_is_space(c)) return true;
    if ((standardize & TFRS_TEXT_STRIP_PUNCTUATION) && text_is_punct(c)) return false;
    if ((standardize & TFRS_TEXT_LOWER) && c - 65u <= 25u) c += 32u;
    word |= (uint64_t)c << ((flen & 7) * 8);
    if ((++flen & 7) == 0) {
      sip.absorb(word);
      word = 0;
    }
    return false;
  }

  // The bytes [a, b) of the string, fetched by `byte_at`.  The inner loop runs to the end of ONE run, so the lanes
  // of a wave leave it together and finish their tokens -- the SipHash finalisation and the table probe, the
  // expensive part -- side by side; finishing inside a flat loop over bytes would run it once per byte position at
  // which ANY lane's token ends.
  template <typename Fetch>
  __device__ __forceinline__ void consume(int64_t a, int64_t b, int standardize, int split, const Emit &emit,
                                          const typename Emit::Row &row, const Fetch &byte_at) {
    int64_t q = a;
    while (q < b) {
      bool ended = false;
      while (q < b && !ended) {
        ended = feed(byte_at(q), standardize, split);
        ++q;
      }
      if (ended) {
        finish(q - 1, emit, row);
        start = q;
      }
    }
  }
};

struct CountEmit {
  int64_t *counts;
  struct Row {
    int64_t i;
  };
  __device__ __forceinline__ Row begin(int64_t i) const { return Row{i}; }
  __device__ __forceinline__ void token(const Row &, int64_t, uint64_t, int64_t, int64_t) const {}
  __device__ __forceinline__ void end(const Row &row, int64_t count) const { counts[row.i] = count; }
};

struct LookupEmit {
  const vocab_slot_t *table;
  int64_t capacity, empty_value;
  const int64_t *row_splits;   // NULL: dense rows of seq_len
  int64_t seq_len;
  int64_t *out;
  struct Row {
    int64_t pos, room;         // the row's first output element and how many it has
  };
  __device__ __forceinline__ Row begin(int64_t i) const {
    if (!row_splits) return Row{i * seq_len, seq_len};
    const int64_t pos = row_splits[i];
    return Row{pos, row_splits[i + 1] - pos};
  }
  __device__ __forceinline__ void token(const Row &row, int64_t t, uint64_t h, int64_t, int64_t) const {
    if (t >= row.room) return;
    const int64_t value = vocab_probe(table, capacity, (int64_t)h, empty_value);
    out[row.pos + t] = value >= 0 ? 2 + value : 1;
  }
  __device__ __forceinline__ void end(const Row &row, int64_t count) const {
    if (row_splits) return;
    for (int64_t t = count; t < row.room; ++t) out[row.pos + t] = 0;
  }
};

struct SpanEmit {
  const int64_t *row_splits;
  int64_t *fingerprints, *starts, *ends;
  struct Row {
    int64_t pos, room;
  };
  __device__ __forceinline__ Row begin(int64_t i) const {
    const int64_t pos = row_splits[i];
    return Row{pos, row_splits[i + 1] - pos};
  }
  __device__ __forceinline__ void token(const Row &row, int64_t t, uint64_t h, int64_t start, int64_t end) const {
    if (t >= row.room) return;
    fingerprints[row.pos + t] = (int64_t)h;
    starts[row.pos + t] = start;
    ends[row.pos + t] = end;
  }
  __device__ __forceinline__ void end(const Row &, int64_t) const {}
};

template <bool WINDOW, typename Emit>
__global__ void __launch_bounds__(256) text_kernel(const unsigned char *__restrict__ bytes, int64_t n_bytes,
                                                   const int64_t *__restrict__ offsets, int64_t n, int standardize,
                                                   int split, const Emit emit) {
  __shared__ __attribute__((aligned(16))) unsigned char window[WINDOW ? kTextWindow : 16];
  for (int64_t first = (int64_t)blockIdx.x * 256; first < n; first += (int64_t)gridDim.x * 256) {
    const int64_t i = first + threadIdx.x;
    const bool live = i < n;
    int64_t lo = 0, hi = 0;
    typename Emit::Row row{};
    if (live) {
      lo = text_clamp(offsets[i], 0, n_bytes);
      hi = text_clamp(offsets[i + 1], lo, n_bytes);
      row = emit.begin(i);
    }
    Tokeniser<Emit> tok(lo);
    if (WINDOW) {
      // the span of the workgroup's strings: every lane reads the same two offsets, so the loop below is uniform
      const int64_t last = first + 256 < n ? first + 256 : n;
      const int64_t span_lo = text_clamp(offsets[first], 0, n_bytes);
      const int64_t span_hi = text_clamp(offsets[last], span_lo, n_bytes);
      // windows start at 16-byte aligned ADDRESSES: the first one may begin up to 15 bytes before the span (and
      // before the blob, where the guard below loads nothing)
      const int64_t base0 = span_lo - (int64_t)(((uintptr_t)bytes + (uint64_t)span_lo) & 15u);
      int64_t p = lo;
      for (int64_t wbase = base0; wbase < span_hi; wbase += kTextWindow) {
        const int64_t wend = wbase + kTextWindow < span_hi ? wbase + kTextWindow : span_hi;
        for (int64_t g = wbase + (int64_t)threadIdx.x * 16; g < wend; g += 256 * 16) {
          unsigned char *dst = window + (g - wbase);
          if (g >= 0 && g + 16 <= n_bytes) {
            *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(bytes + g);
          } else {
            for (int b = 0; b < 16; ++b) dst[b] = (g + b >= 0 && g + b < n_bytes) ? bytes[g + b] : (unsigned char)0;
          }
        }
        __syncthreads();
        const int64_t a = p > wbase ? p : wbase, b = hi < wend ? hi : wend;
        tok.consume(a, b, standardize, split, emit, row, [&](int64_t q) { return (uint32_t)window[q - wbase]; });
        if (b > a) p = b;
        __syncthreads();
      }
    } else {
      tok.consume(lo, hi, standardize, split, emit, row, [&](int64_t q) { return (uint32_t)bytes[q]; });
    }
    if (live) {
      tok.finish(hi, emit, row);
      emit.end(row, tok.count);
    }
  }
}

}  // namespace tfrs

using namespace tfrs;

// Unset, TFRS_TEXT_VARIANT follows profiles/text_vectorization.jsonl: the window is 2 % ahead at title length and three
// times behind at 200 bytes a string, where a workgroup's span takes several windows and its waves wait for one
// another -- so the window serves while the 256 strings of a workgroup fit ONE window on average (64 bytes a string).
static inline bool text_window_variant(int64_t n_bytes, int64_t n) {
  const char *v = option("TFRS_TEXT_VARIANT");
  if (v && v[0] == 'w') return true;
  if (v && v[0] == 'd') return false;
  return n_bytes <= (n + 255) / 256 * (int64_t)kTextWindow;
}

template <typename Emit>
static int text_launch(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                       int standardize, int split, const Emit &emit, void *stream) {
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kTextMaxBlocks)));
  if (text_window_variant(n_bytes, n))
    hipLaunchKernelGGL((text_kernel<true, Emit>), grid, dim3(256), 0, (hipStream_t)stream, bytes, n_bytes, offsets,
                       n, standardize, split, emit);
  else
    hipLaunchKernelGGL((text_kernel<false, Emit>), grid, dim3(256), 0, (hipStream_t)stream, bytes, n_bytes, offsets,
                       n, standardize, split, emit);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

// the checks every entry shares; `bytes` may be NULL for an empty blob, which no lane ever reads
#define TFRS_TEXT_CHECK_INPUT(name)                                                                              \
  TFRS_CHECK_ARG(n >= 0 && n_bytes >= 0, name ": bad count");                                                    \
  TFRS_CHECK_ARG(standardize >= 0 && standardize <= (TFRS_TEXT_LOWER | TFRS_TEXT_STRIP_PUNCTUATION) &&           \
                     (split == TFRS_TEXT_SPLIT_NONE || split == TFRS_TEXT_SPLIT_WHITESPACE),                     \
                 name ": bad standardize / split code (got %d, %d)", standardize, split)

extern "C" int tfrs_text_count_tokens(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                                      int standardize, int split, int64_t *counts, void *stream) {
  TFRS_TEXT_CHECK_INPUT("text_count_tokens");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG((bytes || n_bytes == 0) && offsets && counts, "text_count_tokens: NULL pointer");
  return text_launch(bytes, n_bytes, offsets, n, standardize, split, CountEmit{counts}, stream);
}

extern "C" int tfrs_text_vectorize(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                                   int standardize, int split, const void *table, int64_t capacity, int64_t n_tokens,
                                   int64_t empty_value, const int64_t *row_splits, int64_t seq_len, int64_t *out,
                                   void *stream) {
  TFRS_TEXT_CHECK_INPUT("text_vectorize");
  TFRS_CHECK_ARG(n_tokens >= 0 && capacity >= 1 && (capacity & (capacity - 1)) == 0 && n_tokens <= capacity / 2,
                 "text_vectorize: capacity must be a power of two >= 2 * n_tokens (got capacity %lld, n_tokens %lld)",
                 (long long)capacity, (long long)n_tokens);
  TFRS_CHECK_ARG(empty_value >= -1 && empty_value < n_tokens, "text_vectorize: bad index layout");
  TFRS_CHECK_ARG(row_splits || seq_len >= 1, "text_vectorize: the dense route needs seq_len >= 1 (got %lld)",
                 (long long)seq_len);
  TFRS_CHECK_ARG(table && ((uintptr_t)table) % 16 == 0, "text_vectorize: table must be non-NULL and 16-byte aligned");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG((bytes || n_bytes == 0) && offsets && out, "text_vectorize: NULL pointer");
  return text_launch(bytes, n_bytes, offsets, n, standardize, split,
                     LookupEmit{(const vocab_slot_t *)table, capacity, empty_value, row_splits, seq_len, out}, stream);
}

extern "C" int tfrs_text_token_spans(const unsigned char *bytes, int64_t n_bytes, const int64_t *offsets, int64_t n,
                                     int standardize, int split, const int64_t *row_splits, int64_t *fingerprints,
                                     int64_t *starts, int64_t *ends, void *stream) {
  TFRS_TEXT_CHECK_INPUT("text_token_spans");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG((bytes || n_bytes == 0) && offsets && row_splits && fingerprints && starts && ends,
                 "text_token_spans: NULL pointer");
  return text_launch(bytes, n_bytes, offsets, n, standardize, split, SpanEmit{row_splits, fingerprints, starts, ends},
                     stream);
}
