// The small pieces the lookups (embedding.hip), the sparse updates (sparse_update.h) and the row-wise rule
// (table_rules.h) all use: an id of either width, the capped grid, and the float4-or-scalar access to a chunk of a row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfrs {

template <typename IdT>
__device__ __forceinline__ int64_t load_id(const void *ids, int64_t i) {
  return (int64_t) reinterpret_cast<const IdT *>(ids)[i];
}

inline unsigned grid_for(int64_t total_threads, int64_t cap = 256 * 8) {
  int64_t blocks = (total_threads + 255) / 256;  // default cap: 8 workgroups per CU, grid-stride beyond
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4 *p) {
  const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4 *>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void nt_store4(const float4 &x, float4 *p) {
  nt_f4 v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, reinterpret_cast<nt_f4 *>(p));
}

// One chunk of a row: VEC = 4 a 16-byte piece (p is 16-byte aligned), VEC = 1 a float.  NT: with the non-temporal hint
// (only the float4 form has one).
template <int VEC, bool NT>
__device__ __forceinline__ void vec_load(const float *p, float (&r)[VEC]) {
  if (VEC == 4) {
    const float4 e = NT ? nt_load4(reinterpret_cast<const float4 *>(p)) : *reinterpret_cast<const float4 *>(p);
    r[0] = e.x; r[1 % VEC] = e.y; r[2 % VEC] = e.z; r[3 % VEC] = e.w;
  } else {
    r[0] = *p;
  }
}
template <int VEC, bool NT>
__device__ __forceinline__ void vec_store(float *p, const float (&r)[VEC]) {
  if (VEC == 4) {
    const float4 e = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    if (NT) nt_store4(e, reinterpret_cast<float4 *>(p));
    else *reinterpret_cast<float4 *>(p) = e;
  } else {
    *p = r[0];
  }
}

}  // namespace tfrs
