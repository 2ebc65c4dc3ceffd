// The row quantize of the e4m3 KV cache, one definition for every kernel that
// writes cache rows (kv_cache_fp8.hip, qkv_cache_write.hip).  The format is
// described at the top of kv_cache_fp8.hip.
//
// A row of D values is held by LPR = Dp/8 adjacent lanes, 8 fp32 values each
// (zeros in lanes past D and in the lanes of a skipped row, which still take
// part in the shuffles).  Three steps:
//   kv_row_amax_bits  integer max over the |x| bit patterns of the row (NaN >
//                     Inf > every finite value, so one reduction also finds a
//                     non-finite row), by xor shuffles inside the lane group
//   kv_row_scale      amax / 448; 1 for an all-zero row; NaN for a bad row
//   kv_row_pack       this lane's 8 bytes e4m3_rne(x / scale), saturating;
//                     0x7F throughout in a bad row
#pragma once

#include "fused_math.h"

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int LPR>
__device__ __forceinline__ unsigned int kv_row_amax_bits(const float (&f)[8]) {
  unsigned int abits = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    abits = max(abits, __float_as_uint(f[j]) & 0x7fffffffu);
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1)
    abits = max(abits, (unsigned int)__shfl_xor((int)abits, off, 64));
  return abits;
}

// the row holds a NaN or an Inf
__device__ __forceinline__ bool kv_row_bad(unsigned int abits) {
  return abits >= 0x7f800000u;
}

__device__ __forceinline__ float kv_row_scale(unsigned int abits) {
  return kv_row_bad(abits) ? __uint_as_float(0x7fc00000u)
         : abits == 0u     ? 1.0f
                           : __uint_as_float(abits) / 448.0f;
}

__device__ __forceinline__ u32x2 kv_row_pack(const float (&f)[8],
                                             unsigned int abits, float scale) {
  u32x2 bytes = {0x7f7f7f7fu, 0x7f7f7f7fu};
  if (!kv_row_bad(abits)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned int lo =
          cvt2_fp8<false>(f[4 * h] / scale, f[4 * h + 1] / scale);
      const unsigned int hi =
          cvt2_fp8<false>(f[4 * h + 2] / scale, f[4 * h + 3] / scale);
      bytes[h] = lo | (hi << 16);
    }
  }
  return bytes;
}
