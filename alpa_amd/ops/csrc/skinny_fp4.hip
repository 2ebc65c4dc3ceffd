// MXFP4 decode GEMV for gfx950: y[M,N] = x[M,K] @ W[N,K]^T (+ bias), M <= 8,
// W stored as e2m1 nibbles with one e8m0 scale per 32 k (4.25 bits a weight;
// format, packed layout and dequantization: skinny_fp4.h).  Weight-only: x is
// bf16 and the nibbles become the exact bf16 values in registers, so the sums
// are those of the bf16 kernel over the dequantized weights.
//
// Work split, after skinny_gemm.hip: a lane owns one weight row, a wave 64
// consecutive rows, a workgroup (1 wave) those rows over one k-slice of K/S;
// grid (N/64, S).  The workgroup's x slice is staged in LDS exactly as there
// (stage_x: pair-major, read back with wave-uniform ds_read_b64, broadcast).
//
// Loads: a lane's 16-byte load is ONE whole 32-k block of its row (64 lanes =
// one contiguous 1 KB of wq[K/32][N][16]), and the 8 scale bytes of the 8
// blocks of a pipeline round are one 8-byte load (sq[K/256][N][8]).
//
// Pipeline: a round is 8 blocks = 256 k: 8 independent 16-byte loads and the
// scale load, 136 bytes a lane, like the bf16 kernel's 8-deep rounds (one
// outstanding load runs at HBM latency, not bandwidth: that kernel's v1).
// Nibbles carry 4x the k of bf16 bytes, so a round's VALU work (128 converts
// and 128*MT dot2) is 4x as long per byte: to keep the loads ahead of it the
// rounds are double-buffered in registers.  Round 0 is issued before x is
// staged, round r+1 before round r is consumed; the last round is peeled so
// that no refill sits under a condition.
//
// Per block: 16 v_cvt_scalef32_pk_bf16_fp4 make its 16 bf16 pairs once, then
// per token 8 ds_read_b64 and 16 v_dot2_f32_bf16 into 4 accumulators that
// live across the whole slice (acc[MT][4], summed once at the end).
//
// Split-K as in skinny_gemm.hip: fp32 partials part[S, MT, N] are stored (no
// zeroing, no atomics) and skinny_finalize_kernel reduces them in fixed order,
// adds bias and rounds to bf16.  No scale is applied there or here.
//
// Envelope, next to the bf16 kernel's (N % 64, K % (8*S), K/8/S % 8):
//   N % 64 == 0, K % 256 == 0, S divides K/256 (a k-slice is whole 32-k
//   blocks and whole 8-block rounds), M <= 8 (tiers MT = 4, 8) and the LDS
//   slice (K/S) * 2 * MT bytes <= 64 KB.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950):
//   MT = 4: 80 VGPRs, MT = 8: 94 VGPRs; no AGPRs, no scratch, no static LDS
//   (the x slice is dynamic: (K/S) * 2 * MT bytes).
#include "common.h"
#include "launchers.h"
#include "skinny_dot2.h"
#include "skinny_fp4.h"

#define F4_UNR 8  // 32-k blocks per pipeline round

struct Fp4Round {
  u32x4_t w[F4_UNR];  // one block each
  u32x2_t s;          // their 8 scale bytes
};

__device__ __forceinline__ void load_round(Fp4Round& r, const u32x4_t* w,
                                           const u32x2_t* s, int64_t N) {
#pragma unroll
  for (int u = 0; u < F4_UNR; ++u) r.w[u] = w[(int64_t)u * N];
  r.s = *s;
}

// acc += the round's 8 blocks . x; xb is the round's first pair group in LDS
template <int MT>
__device__ __forceinline__ void dot_round(const Fp4Round& r, const i32x2* xb,
                                          float (&acc)[MT][4]) {
#pragma unroll
  for (int u = 0; u < F4_UNR; ++u) {
    const float sf = fp4_scale(r.s[u >> 2], u & 3);
    u32x4_t p[4];  // p[d][j]: k pair 8*d + 2*j of the block
#pragma unroll
    for (int d = 0; d < 4; ++d) p[d] = fp4x8_to_bf16(r.w[u][d], sf);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      i32x2 a[4], b[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        a[d] = xb[((u * 4 + d) * 2 + 0) * MT + m];
        b[d] = xb[((u * 4 + d) * 2 + 1) * MT + m];
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        acc[m][0] = dot2_bf16(pair_lo(p[d][0]), pair_lo(a[d][0]), acc[m][0]);
        acc[m][1] = dot2_bf16(pair_lo(p[d][1]), pair_lo(a[d][1]), acc[m][1]);
        acc[m][2] = dot2_bf16(pair_lo(p[d][2]), pair_lo(b[d][0]), acc[m][2]);
        acc[m][3] = dot2_bf16(pair_lo(p[d][3]), pair_lo(b[d][1]), acc[m][3]);
      }
    }
  }
}

template <int MT>
__launch_bounds__(64, 1)
__global__ void skinny_fp4_kernel(
    const u32x4_t* __restrict__ wq,  // [K/32, N] blocks of 32 nibbles
    const u32x2_t* __restrict__ sq,  // [K/256, N] groups of 8 scale bytes
    const short* __restrict__ x,     // [MT, K] bf16 (padded rows zero)
    float* __restrict__ part,        // [S, MT, N] fp32 (overwritten)
    int64_t N, int64_t K, int rounds) {
  extern __shared__ i32x2 xs[];
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * rounds;  // first round of the slice
  const u32x4_t* wrow = wq + r0 * F4_UNR * N + row;
  const u32x2_t* srow = sq + r0 * N + row;
  const int64_t wstep = (int64_t)F4_UNR * N;
  Fp4Round cur, nxt;
  load_round(cur, wrow, srow, N);
  // a round is 32 of stage_x's 8-k groups
  stage_x<MT>(x, xs, K, (int)(r0 * 32), rounds * 32);
  float acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m][j] = 0.f;
  int r = 0;
  for (; r < rounds - 1; ++r) {
    load_round(nxt, wrow + (r + 1) * wstep, srow + (int64_t)(r + 1) * N, N);
    dot_round<MT>(cur, xs + r * 64 * MT, acc);
    cur = nxt;
  }
  dot_round<MT>(cur, xs + r * 64 * MT, acc);
  float* out = part + ((int64_t)blockIdx.y * MT) * N + row;
#pragma unroll
  for (int m = 0; m < MT; ++m)
    out[(int64_t)m * N] = (acc[m][0] + acc[m][1]) + (acc[m][2] + acc[m][3]);
}

extern "C" {

// x is [MT, K] with rows M..MT-1 zero, part [splits, MT, N];
// hipErrorInvalidValue outside the envelope (see launchers.h)
hipError_t launch_skinny_fp4(const void* wq, const void* sq, const void* x,
                             float* part, const void* bias_or_null, void* y,
                             int64_t M, int64_t MT, int64_t N, int64_t K,
                             int splits, hipStream_t stream) {
  if (M < 1 || M > MT || (MT != 4 && MT != 8) || N <= 0 || N % 64 ||
      K <= 0 || K % 256 || splits < 1 || (K / 256) % splits)
    return hipErrorInvalidValue;
  const int rounds = (int)(K / 256 / splits);
  const size_t lds = (size_t)rounds * 64 * MT * sizeof(i32x2);
  if (lds > SKINNY_FP4_LDS_MAX) return hipErrorInvalidValue;
  dim3 grid((uint32_t)(N / 64), (uint32_t)splits);
  if (MT == 4)
    skinny_fp4_kernel<4><<<grid, dim3(64), lds, stream>>>(
        (const u32x4_t*)wq, (const u32x2_t*)sq, (const short*)x, part, N, K,
        rounds);
  else
    skinny_fp4_kernel<8><<<grid, dim3(64), lds, stream>>>(
        (const u32x4_t*)wq, (const u32x2_t*)sq, (const short*)x, part, N, K,
        rounds);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int64_t total = M * N;
  skinny_finalize_kernel<<<dim3((uint32_t)((total + 255) / 256)), dim3(256),
                           0, stream>>>(part, (const short*)bias_or_null,
                                        (short*)y, MT, M, N, splits);
  return hipGetLastError();
}

}  // extern "C"
