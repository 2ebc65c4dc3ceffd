// MXFP4 weights as the two fp4 skinny kernels read them (skinny_fp4.hip up to
// 8 tokens, skinny_mfma_fp4.hip for 9..64), and their dequantization.
//
// Format (OCP MX): a weight is an e2m1 code sign<<3 | exp<<1 | mant (values
// +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}); 32 consecutive k of a row share one e8m0
// scale byte E, factor 2^(E-127), 2 <= E <= 252.
//
// Packed layout, one for both kernels (ops.mxfp4_pack builds it):
//   wq [K/32][N][16] bytes: the unit of row n and block b is that block's 32
//      nibbles, k ascending, even k in the low nibble -- 4 dwords of 8 k each.
//      For one block, 64 consecutive rows are one contiguous 1 KB.
//   sq [K/256][N][8] bytes: byte j is the scale of row n, block 8*g + j.
// A 16-byte load is one whole block of one row under ONE scale, in both
// kernels: the lane-per-row kernel's lane takes its row's unit (64 lanes =
// one coalesced 1 KB), and the MFMA kernel's lane (lo, hi) takes the unit of
// row lo, block hi of a 128-k chunk, whose 4 dwords feed 4 MFMAs (a wave's
// load instruction covers four 256-byte runs, whole cache lines).  The 8
// scales of a row's 256 k are one 8-byte load in either kernel.
//
// Dequantization: e2m1 * 2^(E-127) is a bf16 exactly (one mantissa bit, the
// scale only moves the exponent, and E's range keeps it normal), so
// v_cvt_scalef32_pk_bf16_fp4 -- two nibbles of a byte to a bf16 pair, scaled
// by the exponent of an fp32 -- is exact: the bit pattern is the nibble's
// with E - 127 added to the exponent field, 0.5 (e2m1's subnormal) a normal
// 2^(E-128), zeros staying zeros.  One instruction per pair, no float
// multiply, nothing to round; no scale is left for the accumulators.
#pragma once

#include "common.h"

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 hwbf16x2 __attribute__((ext_vector_type(2)));

// defined in skinny_gemm.hip; part is [splits, MT, N], rows 0..M-1 are read
__global__ void skinny_finalize_kernel(const float* __restrict__ part,
                                       const short* __restrict__ bias,
                                       short* __restrict__ y, int64_t MT,
                                       int64_t M, int64_t N, int splits);

// the fp32 2^(E-127) of scale byte j (0..3) of a dword of scale bytes
__device__ __forceinline__ float fp4_scale(uint32_t s, int j) {
  return __uint_as_float(((s >> (8 * j)) & 0xffu) << 23);
}

// 8 nibbles (k ascending from bit 0) -> 4 bf16 pairs, low half = even k
__device__ __forceinline__ u32x4_t fp4x8_to_bf16(uint32_t d, float scale) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(
      uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0));
  r[1] = __builtin_bit_cast(
      uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1));
  r[2] = __builtin_bit_cast(
      uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2));
  r[3] = __builtin_bit_cast(
      uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3));
  return r;
}
