// What the lane-per-row skinny kernels share (skinny_gemm.hip, and
// skinny_fp4.hip over MXFP4 weights): the packed-pair dot product and the
// x slice staged in LDS.
#pragma once

#include "common.h"

typedef short bf16x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// dot of a packed bf16 pair with accumulate (v_dot2_f32_bf16)
__device__ __forceinline__ float dot2_bf16(bf16x2 a, bf16x2 b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(a, b, acc, false);
}

__device__ __forceinline__ bf16x2 mk2(short a, short b) {
  bf16x2 r;
  r[0] = a;
  r[1] = b;
  return r;
}

__device__ __forceinline__ bf16x2 pair_lo(int v) {
  bf16x2 r;
  r[0] = (short)(v & 0xffff);
  r[1] = (short)((unsigned int)v >> 16);
  return r;
}

// Stage x[0:MT, kg0*8 : (kg0+rounds)*8] into LDS, transposed to
// half-round-major: xs[(r*2 + h) * MT + m] = i32x2 holding k-pairs
// (4h, 4h+1) of round r for row m.  Coalesced 16-B global reads.
template <int MT>
__device__ __forceinline__ void stage_x(const short* __restrict__ x,
                                        i32x2* xs, int64_t K, int kg0,
                                        int rounds) {
  for (int i = threadIdx.x; i < MT * rounds; i += 64) {
    const int m = i / rounds, r = i - (i / rounds) * rounds;
    bf16x4 lo = *reinterpret_cast<const bf16x4*>(
        x + (int64_t)m * K + ((int64_t)(kg0 + r)) * 8);
    bf16x4 hi = *reinterpret_cast<const bf16x4*>(
        x + (int64_t)m * K + ((int64_t)(kg0 + r)) * 8 + 4);
    i32x2 a, b;
    a[0] = ((int)(unsigned short)lo[0]) | ((int)(unsigned short)lo[1] << 16);
    a[1] = ((int)(unsigned short)lo[2]) | ((int)(unsigned short)lo[3] << 16);
    b[0] = ((int)(unsigned short)hi[0]) | ((int)(unsigned short)hi[1] << 16);
    b[1] = ((int)(unsigned short)hi[2]) | ((int)(unsigned short)hi[3] << 16);
    xs[(r * 2 + 0) * MT + m] = a;
    xs[(r * 2 + 1) * MT + m] = b;
  }
  __syncthreads();
}
