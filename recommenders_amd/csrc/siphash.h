// siphash.h -- the SipHash-2-4 state shared by hashing.hip (salted buckets, fingerprints of packed strings) and
// text.hip (fingerprints of tokens as they are cut out of a string).
#pragma once

#include "common.h"

namespace tfrs {

struct Sip {
  uint64_t v0, v1, v2, v3;
  __device__ __forceinline__ Sip(uint64_t k0, uint64_t k1)
      : v0(k0 ^ 0x736f6d6570736575ull), v1(k1 ^ 0x646f72616e646f6dull),
        v2(k0 ^ 0x6c7967656e657261ull), v3(k1 ^ 0x7465646279746573ull) {}
  static __device__ __forceinline__ uint64_t rotl(uint64_t x, int b) {
    return (x << b) | (x >> (64 - b));
  }
  __device__ __forceinline__ void round() {
    v0 += v1; v1 = rotl(v1, 13) ^ v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16) ^ v2;
    v0 += v3; v3 = rotl(v3, 21) ^ v0;
    v2 += v1; v1 = rotl(v1, 17) ^ v2; v2 = rotl(v2, 32);
  }
  __device__ __forceinline__ void absorb(uint64_t m) {
    v3 ^= m;
    round();
    round();
    v0 ^= m;
  }
  __device__ __forceinline__ uint64_t finish() {
    v2 ^= 0xff;
    round();
    round();
    round();
    round();
    return v0 ^ v1 ^ v2 ^ v3;
  }
};

// The full 64-bit SipHash-2-4 of every packed string under ONE fixed key (the SipHash paper's test key
// 00 01 .. 0f): the keys of StringLookup's vocabulary table (vocab.hip).
constexpr uint64_t kFingerprintK0 = 0x0706050403020100ull, kFingerprintK1 = 0x0f0e0d0c0b0a0908ull;

}  // namespace tfrs
