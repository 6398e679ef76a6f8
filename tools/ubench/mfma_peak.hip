// Saturating MFMA loop (round 5): what the fp16 matrix pipe of this chip sustains when
// NOTHING but MFMAs is issued -- NACC independent 32 x 32 output tiles per wave that persist over the whole kernel
// (no re-zeroing: one dependency chain per accumulator), operands in registers, 1 / 2 / 4 waves per SIMD -- on
// all-zero operands (must reach the guide's 2495 TFLOP/s before anything else measured with it is called a
// ceiling) and on random operands (the clock follows the power the operand data draws).
// Two instruction shapes at the SAME output tile per wave and the same flop per iteration:
//   32x32  v_mfma_f32_32x32x16_{f16,bf16}: one 16-register accumulator per tile, 32 cycles per instruction and SIMD
//   16x16  v_mfma_f32_16x16x32_{f16,bf16}: four 4-register accumulators per tile, 16 cycles per instruction and SIMD
// and, in the "A from LDS" rows, the A operand re-read from LDS with ds_read_b128 at every K step (one 16-byte read
// per lane and 32 rows x 16 features for either shape), which is what the top-K scan does with its candidates.
// The shader clock is logged beside every rate: cycles of s_memtime (clock64) over the kernel against the 100 MHz
// wall clock, and the clock implied by the MFMA count.
//   hipcc --offload-arch=gfx950 -O3 mfma_peak.hip -o mfma_peak && ./mfma_peak
#include <hip/hip_runtime.h>
#pragma clang diagnostic ignored "-Wunused-result"
#pragma clang diagnostic ignored "-Wunused-value"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <bool BF16>
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) {
  if constexpr (BF16)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
template <bool BF16>
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
  if constexpr (BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// SHAPE = 32: per iteration 16 K-steps of 16, tile n = a[c & 3] x b[n][0].
// SHAPE = 16: per iteration 8 K-steps of 32, tile n = 2 row halves (a[2 * (c & 1) + rh]) x 2 column halves (b[n][ch]).
// LDSA: a[] is not kept in registers; the fragment of every K step is read from LDS (offset made opaque per read so
// that the compiler can neither hoist nor merge the reads).
template <int NACC, int SHAPE, bool BF16, bool LDSA>
__global__ void __launch_bounds__(256) sat(const f16x8 *in, float *out, long long *clk, int iters) {
  __shared__ f16x8 lds[4 * 256];
  f16x8 a[4], b[NACC][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = in[threadIdx.x + 256 * i];
    lds[threadIdx.x + 256 * i] = a[i];
  }
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    b[i][0] = in[threadIdx.x + 256 * (4 + i)];
    b[i][1] = in[((threadIdx.x + 64) & 255) + 256 * (4 + i)];
  }
  __syncthreads();
  f32x16 acc[NACC];
#pragma unroll
  for (int n = 0; n < NACC; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  int off = threadIdx.x;
  const long long c0 = clock64(), w0 = wall_clock64();
  for (int it = 0; it < iters; ++it) {
    if constexpr (SHAPE == 32) {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        f16x8 av = a[c & 3];
        if constexpr (LDSA) {
          asm volatile("" : "+v"(off));
          av = lds[off + 256 * (c & 3)];
        }
#pragma unroll
        for (int n = 0; n < NACC; ++n) acc[n] = mfma32<BF16>(av, b[n][0], acc[n]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        f16x8 av[2] = {a[2 * (c & 1)], a[2 * (c & 1) + 1]};
        if constexpr (LDSA) {
          asm volatile("" : "+v"(off));
          av[0] = lds[off + 256 * (2 * (c & 1))];
          av[1] = lds[off + 256 * (2 * (c & 1) + 1)];
        }
#pragma unroll
        for (int n = 0; n < NACC; ++n)
#pragma unroll
          for (int rh = 0; rh < 2; ++rh)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
              f32x4 q = {acc[n][8 * rh + 4 * ch], acc[n][8 * rh + 4 * ch + 1], acc[n][8 * rh + 4 * ch + 2],
                         acc[n][8 * rh + 4 * ch + 3]};
              q = mfma16<BF16>(av[rh], b[n][ch], q);
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[n][8 * rh + 4 * ch + r] = q[r];
            }
      }
    }
  }
  const long long c1 = clock64(), w1 = wall_clock64();
  float res = 0.f;
#pragma unroll
  for (int n = 0; n < NACC; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) res += acc[n][r];
  out[blockIdx.x * 256 + threadIdx.x] = res;
  if (blockIdx.x == 0 && threadIdx.x == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; }
}

template <int NACC, int SHAPE, bool BF16, bool LDSA = false>
void run(const f16x8 *in, float *out, long long *clk, int waves_per_simd, int iters) {
  const int wgs = 256 * waves_per_simd;        // 256 CUs x (4 waves = 1 per SIMD) per workgroup
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  sat<NACC, SHAPE, BF16, LDSA><<<wgs, 256>>>(in, out, clk, 100);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  sat<NACC, SHAPE, BF16, LDSA><<<wgs, 256>>>(in, out, clk, iters);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  long long h[2]; hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
  // per iteration and tile: 16 instructions of 32x32x16 (32 cycles) or 32 of 16x16x32 (16 cycles): 2^19 flop either way
  const int per_tile = SHAPE == 32 ? 16 : 32, cyc = SHAPE == 32 ? 32 : 16;
  const double mfma_per_simd = (double)waves_per_simd * iters * (double)per_tile * NACC;
  const double flop = mfma_per_simd * 1024.0 * (SHAPE == 32 ? 32768.0 : 16384.0);   // 1024 SIMDs
  printf("%-4s %-8s %-10s %d tiles, %d wave(s)/SIMD: %8.3f ms  %7.0f TFLOP/s  (%.3f of 2500)   clock: s_memtime %.0f MHz, "
         "implied by %d cycles per MFMA %.0f MHz\n", BF16 ? "bf16" : "fp16", SHAPE == 32 ? "32x32x16" : "16x16x32",
         LDSA ? "A from LDS" : "registers", NACC, waves_per_simd, ms, flop / ms / 1e9, flop / ms / 1e9 / 2500.0,
         (double)h[0] / ((double)h[1] / 100.0), cyc, mfma_per_simd * cyc / (ms * 1e3));
  hipEventDestroy(e0); hipEventDestroy(e1);
}

template <int SHAPE>
void rows(const f16x8 *in, float *out, long long *clk, const void *h16, const void *hb16, int iters) {
  hipMemcpy((void *)in, h16, 256 * 12 * 16, hipMemcpyHostToDevice);
  for (int w : {1, 2}) run<4, SHAPE, false>(in, out, clk, w, iters / w);   // (32x32: 132 registers, 3 waves fit, 4 do not)
  run<8, SHAPE, false>(in, out, clk, 1, iters / 2);
  run<2, SHAPE, false>(in, out, clk, 4, iters / 2);                           // 4 waves per SIMD
  run<2, SHAPE, false, true>(in, out, clk, 2, iters);                         // the scan's structure: two tiles per A fragment
  run<2, SHAPE, false, true>(in, out, clk, 4, iters / 2);
  hipMemcpy((void *)in, hb16, 256 * 12 * 16, hipMemcpyHostToDevice);
  for (int w : {1, 2}) run<4, SHAPE, true>(in, out, clk, w, iters / w);
  run<2, SHAPE, true, true>(in, out, clk, 4, iters / 2);
}

int main(int argc, char **argv) {
  f16x8 *in; float *out; long long *clk;
  hipMalloc(&in, 256 * 12 * sizeof(f16x8)); hipMalloc(&out, 1024 * 256 * 4); hipMalloc(&clk, 16);
  _Float16 *h = (_Float16 *)malloc(256 * 12 * 16);
  unsigned short *hb = (unsigned short *)malloc(256 * 12 * 16);
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  const int reps = argc > 2 ? atoi(argv[2]) : 2;      // the two shapes alternate `reps` times per operand kind
  for (const char *mode : {"zeros", "random", "random/8"}) {
    srand(1);
    for (int i = 0; i < 256 * 12 * 8; ++i) {
      float v = mode[0] == 'z' ? 0.f : (rand() % 2001 - 1000) / 1000.0f;
      if (strlen(mode) > 6) v *= 0.125f;               // the scan's operands: corpus rows scaled into [-1, 1] / sqrt(64)
      h[i] = (_Float16)v;
      unsigned u; memcpy(&u, &v, 4);
      hb[i] = (unsigned short)(u >> 16);
    }
    printf("---- operands: %s (fp16 / bf16 hold the same values)\n", mode);
    for (int r = 0; r < reps; ++r) {
      rows<32>(in, out, clk, h, hb, iters);
      rows<16>(in, out, clk, h, hb, iters);
    }
  }
  return 0;
}
