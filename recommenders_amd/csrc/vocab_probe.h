// vocab_probe.h -- one probe of the vocabulary table, shared by vocab.hip (ids -> indices) and text.hip (tokens cut
// out of a string -> indices).  The table's layout and its rules are stated at the head of vocab.hip.
#pragma once

#include "common.h"

namespace tfrs {

constexpr int64_t kVocabEmpty = TFRS_VOCAB_EMPTY_KEY;

typedef long long vocab_slot_t __attribute__((ext_vector_type(2)));   // .x = key, .y = value

// the 64-bit finalizer of MurmurHash3 (Appleby, public domain): every input bit reaches every output bit
__host__ __device__ __forceinline__ uint64_t vocab_mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// The vocabulary position of `key`, or -1: TFRS_VOCAB_EMPTY_KEY is answered from `empty_value`, every other key by
// linear probing from its home slot until the key or a free slot is met -- after `capacity` steps at the latest.
__device__ __forceinline__ int64_t vocab_probe(const vocab_slot_t *__restrict__ table, int64_t capacity, int64_t key,
                                               int64_t empty_value) {
  const uint64_t mask = (uint64_t)capacity - 1;
  int64_t value = -1;
  if (key == kVocabEmpty) {
    value = empty_value;
  } else {
    uint64_t slot = vocab_mix((uint64_t)key) & mask;
    for (int64_t step = 0; step < capacity; ++step, slot = (slot + 1) & mask) {
      const vocab_slot_t s = table[slot];
      if (s.x == key) {
        value = s.y;
        break;
      }
      if (s.x == kVocabEmpty) break;
    }
  }
  return value;
}

}  // namespace tfrs
