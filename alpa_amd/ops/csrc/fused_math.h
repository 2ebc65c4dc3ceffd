// Device helpers shared by the elementwise, quantize and fused-quantize
// kernels.  One definition each: the fused kernels in fp8_fused.hip must
// produce the bytes of bias_gelu.hip / layernorm.hip followed by
// fp8_quant.hip, so they evaluate the very same inline functions.
#pragma once

#include "common.h"

// tanh-GeLU via the sigmoid identity: 0.5x(1+tanh(z)) == x*sigmoid(2z),
// evaluated with ONE hardware __expf instead of libm tanhf (the tanh
// path ran the elementwise kernels 1.7-1.9x off the HBM roofline —
// VALU-bound on the polynomial tanh expansion).  Same function, only
// the evaluation differs; bf16 outputs agree to rounding.
__device__ __forceinline__ float gelu_sigmoid(float x) {
  const float k2 = 2.0f * 0.7978845608028654f;
  float z2 = k2 * (x + 0.044715f * x * x * x);
  return 1.0f / (1.0f + __expf(-z2));
}

__device__ __forceinline__ float gelu_f(float x) {
  return x * gelu_sigmoid(x);
}

// e4m3: clamp 448; e5m2 (ISA name bf8): clamp 57344. RNE conversion via
// the packed hardware converters.
template <bool E5M2>
__device__ __forceinline__ unsigned short cvt2_fp8(float a, float b) {
  a = __builtin_amdgcn_fmed3f(a, E5M2 ? 57344.f : 448.f,
                              E5M2 ? -57344.f : -448.f);
  b = __builtin_amdgcn_fmed3f(b, E5M2 ? 57344.f : 448.f,
                              E5M2 ? -57344.f : -448.f);
  unsigned int packed =
      E5M2 ? __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false)
           : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return (unsigned short)(packed & 0xffff);
}

__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  // positive floats compare correctly as uints.  Guard with a plain
  // read first: with ~80k blocks all reducing into ONE scalar, the
  // serialized same-address atomics would otherwise dominate; after
  // the first few blocks the running max is usually already >= v and
  // the atomic is skipped (monotonic, so the race is benign).
  volatile unsigned int* a = reinterpret_cast<volatile unsigned int*>(addr);
  if (__float_as_uint(v) > *a)
    atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

typedef unsigned char u8x8 __attribute__((ext_vector_type(8)));
typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));

// delayed scaling: the multiplier every quantize kernel applies
__device__ __forceinline__ float fp8_inv_scale(const float* scale) {
  return 1.0f / fmaxf(*scale, 1e-12f);
}

// 2*K values -> amax, and K byte pairs of f * inv in out[0 .. 2*K).  `f` and
// `out` are anything indexable (arrays, ext vectors, an LDS pointer).
template <bool E5M2, int K, typename In, typename Out>
__device__ __forceinline__ void fp8_pack(const In& f, float inv, float& amax,
                                         Out&& out) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    amax = fmaxf(fmaxf(amax, fabsf(f[2 * j])), fabsf(f[2 * j + 1]));
    unsigned short p = cvt2_fp8<E5M2>(f[2 * j] * inv, f[2 * j + 1] * inv);
    out[2 * j] = (unsigned char)(p & 0xff);
    out[2 * j + 1] = (unsigned char)(p >> 8);
  }
}

// One 64x64 tile of the dual-layout quantize: q [M, N] row-major and
// qt [N, M] transposed from one pass over the source, amax into *amax_out.
// Grid (ceil(N/64), ceil(M/64)), 256 threads.  `load(row, col)` returns the
// four fp32 values of the column quad at (row, col..col+3), and zeros
// outside the tensor, which neither move amax nor get stored.
//
// Phase 1 converts the tile into LDS as fp8 bytes; phases 2/3 drain it with
// 16-BYTE stores per lane (row-major q and transposed qt) so both global
// write streams are fully coalesced — the first cut used 4-byte scattered
// stores and ran 4x off the bandwidth roofline (profiles/prof_fp8 r2).
#define FP8_TILE 64

template <bool E5M2, typename Loader>
__device__ __forceinline__ void fp8_quantize_tile(
    Loader&& load, unsigned char* __restrict__ q,
    unsigned char* __restrict__ qt, const float* __restrict__ scale,
    float* __restrict__ amax_out, int64_t M, int64_t N) {
  const float inv = fp8_inv_scale(scale);
  // +4 bytes: depivot banks
  __shared__ unsigned char tile[FP8_TILE][FP8_TILE + 4];
  const int64_t row0 = (int64_t)blockIdx.y * FP8_TILE;
  const int64_t col0 = (int64_t)blockIdx.x * FP8_TILE;
  const int t = threadIdx.x;           // 256 threads
  const int tc = (t & 15) * 4;         // 4 consecutive cols
  const int tr = t >> 4;               // 16 rows per pass
  const bool interior = (row0 + FP8_TILE <= M) && (col0 + FP8_TILE <= N);
  // a 16-byte store needs a 16-byte row pitch as well as a whole tile
  const bool vec_q = interior && (N % 16 == 0);
  const bool vec_qt = interior && (M % 16 == 0);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = tr + i * 16;
    fp8_pack<E5M2, 2>(load(row0 + r, col0 + tc), inv, amax, &tile[r][tc]);
  }
  __syncthreads();
  const int r = t >> 2;                // 0..63: a row of q, then of qt
  const int c16 = (t & 3) * 16;        // 4 lanes cover one 64-B row
  // phase 2: row-major q
  {
    const int64_t gr = row0 + r;
    if (vec_q) {
      u8x16 v;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[r][c16 + j];
      *reinterpret_cast<u8x16*>(q + gr * N + col0 + c16) = v;
    } else if (gr < M) {
      for (int j = 0; j < 16; ++j)
        if (col0 + c16 + j < N) q[gr * N + col0 + c16 + j] = tile[r][c16 + j];
    }
  }
  // phase 3: transposed qt; r is the original column, c16 the original rows
  {
    const int64_t gq = col0 + r;
    if (vec_qt) {
      u8x16 v;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[c16 + j][r];
      *reinterpret_cast<u8x16*>(qt + gq * M + row0 + c16) = v;
    } else if (gq < N) {
      for (int j = 0; j < 16; ++j)
        if (row0 + c16 + j < M)
          qt[gq * M + row0 + c16 + j] = tile[c16 + j][r];
    }
  }
  __shared__ float red[16];
  amax = block_reduce_max(amax, red);
  if (threadIdx.x == 0) atomic_max_f32(amax_out, amax);
}
