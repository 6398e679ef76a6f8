// vocab.hip -- device-resident vocabulary table behind IntegerLookup / StringLookup.
//
// Replaces the tf.keras.layers.IntegerLookup / StringLookup layers that the reference's tutorials put in
// front of every Embedding: token -> index, unknown tokens to the OOV slots.
//
// The table is open addressing with linear probing over `capacity` (a power of two >= 2 n) slots of 16
// bytes {key, value}: one probe step is one global_load_dwordx4.  A 64-bit mixer of the key picks the home
// slot.  One key value, TFRS_VOCAB_EMPTY_KEY, marks a free slot and is never stored: a vocabulary token or a
// query of that value is answered from a kernel argument instead.
//
// Integer work, latency-bound: a lookup is a chain of dependent random 16-byte reads (1.5 probes expected
// for a hit and 2.5 for a miss at load factor 1/2), so one lane owns one id and the ids in flight hide the
// latency.  Per id: 8 B (or 4 B) read, 8 B written, 16 B per probe.
//
// EVERY probe loop stops after `capacity` steps, whatever the table holds: a malformed table gives wrong
// indices, never a kernel that spins.
#include "common.h"
#include "vocab_probe.h"

namespace tfrs {

constexpr int kVocabMaxBlocks = 2048;   // grid cap: 256 CUs x 8 blocks of 256 lanes, grid-stride beyond

__global__ void __launch_bounds__(256) vocab_clear_kernel(vocab_slot_t *__restrict__ table, int64_t capacity,
                                                          uint32_t *__restrict__ flags) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) *flags = 0u;
  vocab_slot_t e;
  e.x = kVocabEmpty;
  e.y = -1;
  for (int64_t i = first; i < capacity; i += (int64_t)gridDim.x * blockDim.x) table[i] = e;
}

// key i -> value i.  The compare-and-swap on the key word claims a slot; the value is stored plainly after
// it, which is enough because no lookup runs before this launch has ended.  A CAS that returns the lane's
// own key found a duplicate; a lane that finds no slot in `capacity` steps (impossible for a cleared table
// of capacity >= 2 n) reports a full table.
__global__ void __launch_bounds__(256) vocab_insert_kernel(const int64_t *__restrict__ keys, int64_t n,
                                                           int64_t *__restrict__ table, int64_t capacity,
                                                           uint32_t *__restrict__ flags) {
  const uint64_t mask = (uint64_t)capacity - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t key = keys[i];
    if (key == kVocabEmpty) continue;   // answered outside the table (tfrs_vocab_lookup's empty_value)
    uint64_t slot = vocab_mix((uint64_t)key) & mask;
    uint32_t outcome = TFRS_VOCAB_TABLE_FULL;
    for (int64_t step = 0; step < capacity; ++step, slot = (slot + 1) & mask) {
      const int64_t seen = (int64_t)atomicCAS(reinterpret_cast<unsigned long long *>(table + 2 * slot),
                                              (unsigned long long)kVocabEmpty, (unsigned long long)key);
      if (seen == kVocabEmpty) {
        table[2 * slot + 1] = i;
        outcome = 0u;
        break;
      }
      if (seen == key) {
        outcome = TFRS_VOCAB_DUPLICATE_KEY;
        break;
      }
    }
    if (outcome) atomicOr(flags, outcome);
  }
}

template <typename IdT>
__global__ void __launch_bounds__(256) vocab_lookup_kernel(
    const IdT *__restrict__ ids, int64_t n, const vocab_slot_t *__restrict__ table, int64_t capacity,
    int64_t base, int has_mask, int64_t mask_key, int64_t empty_value, int64_t oov_base, int64_t num_oov,
    int oov_unsigned, unsigned long long *__restrict__ unknown, int64_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t key = (int64_t)ids[i];
    if (has_mask && key == mask_key) {
      out[i] = 0;
      continue;
    }
    const int64_t value = vocab_probe(table, capacity, key, empty_value);
    int64_t index;
    if (value >= 0) {
      index = base + value;
    } else {
      if (unknown) atomicAdd(unknown, 1ull);
      if (num_oov == 0) {
        index = -1;
      } else if (num_oov == 1) {
        index = oov_base;
      } else if (oov_unsigned) {
        index = oov_base + (int64_t)((uint64_t)key % (uint64_t)num_oov);
      } else {
        const int64_t r = key % num_oov;   // C++ remainder has the dividend's sign; floormod does not
        index = oov_base + (r < 0 ? r + num_oov : r);
      }
    }
    out[i] = index;
  }
}

}  // namespace tfrs

using namespace tfrs;

static inline unsigned vocab_grid(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kVocabMaxBlocks));
}

static inline bool vocab_capacity_ok(int64_t capacity, int64_t n) {
  return capacity >= 1 && (capacity & (capacity - 1)) == 0 && n <= capacity / 2;
}

extern "C" int tfrs_vocab_build(const int64_t *keys, int64_t n, void *table, int64_t capacity, uint32_t *flags,
                                void *stream) {
  TFRS_CHECK_ARG(n >= 0, "vocab_build: bad count");
  TFRS_CHECK_ARG(vocab_capacity_ok(capacity, n),
                 "vocab_build: capacity must be a power of two >= 2 * n (got capacity %lld, n %lld)",
                 (long long)capacity, (long long)n);
  TFRS_CHECK_ARG(table && flags && (keys || n == 0), "vocab_build: NULL pointer");
  TFRS_CHECK_ARG(((uintptr_t)table) % 16 == 0, "vocab_build: table must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vocab_clear_kernel, dim3(vocab_grid(capacity)), dim3(256), 0, s, (vocab_slot_t *)table,
                     capacity, flags);
  TFRS_LAUNCH_CHECK();
  if (n == 0) return TFRS_OK;
  hipLaunchKernelGGL(vocab_insert_kernel, dim3(vocab_grid(n)), dim3(256), 0, s, keys, n, (int64_t *)table,
                     capacity, flags);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}

extern "C" int tfrs_vocab_lookup(const void *ids, int ids_are_i64, int64_t n, const void *table, int64_t capacity,
                                 int64_t n_tokens, int64_t base, int has_mask, int64_t mask_key,
                                 int64_t empty_value, int64_t oov_base, int64_t num_oov, int oov_unsigned,
                                 int64_t *unknown_count, int64_t *out, void *stream) {
  TFRS_CHECK_ARG(n >= 0 && n_tokens >= 0, "vocab_lookup: bad count");
  TFRS_CHECK_ARG(vocab_capacity_ok(capacity, n_tokens),
                 "vocab_lookup: capacity must be a power of two >= 2 * n_tokens (got capacity %lld, n_tokens %lld)",
                 (long long)capacity, (long long)n_tokens);
  TFRS_CHECK_ARG(num_oov >= 0 && base >= 0 && oov_base >= 0 && empty_value >= -1 && empty_value < n_tokens,
                 "vocab_lookup: bad index layout");
  TFRS_CHECK_ARG(table && ((uintptr_t)table) % 16 == 0, "vocab_lookup: table must be non-NULL and 16-byte aligned");
  if (n == 0) return TFRS_OK;
  TFRS_CHECK_ARG(ids && out, "vocab_lookup: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (ids_are_i64)
    hipLaunchKernelGGL((vocab_lookup_kernel<int64_t>), dim3(vocab_grid(n)), dim3(256), 0, s, (const int64_t *)ids, n,
                       (const vocab_slot_t *)table, capacity, base, has_mask, mask_key, empty_value, oov_base,
                       num_oov, oov_unsigned, (unsigned long long *)unknown_count, out);
  else
    hipLaunchKernelGGL((vocab_lookup_kernel<int32_t>), dim3(vocab_grid(n)), dim3(256), 0, s, (const int32_t *)ids, n,
                       (const vocab_slot_t *)table, capacity, base, has_mask, mask_key, empty_value, oov_base,
                       num_oov, oov_unsigned, (unsigned long long *)unknown_count, out);
  TFRS_LAUNCH_CHECK();
  return TFRS_OK;
}
