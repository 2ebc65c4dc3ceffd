// MXFP4 MFMA skinny GEMM for gfx950: y[M,N] = x[M,K] @ W[N,K]^T (+ bias) for
// decode batches of 9 <= M <= 64 tokens, over the packed MXFP4 weights of the
// lane-per-row kernel (skinny_fp4.hip; format, layout and dequantization in
// skinny_fp4.h): wq[K/32][N][16] nibble blocks, sq[K/256][N][8] scale bytes.
// Weight-only: the nibbles become the exact bf16 values in registers and feed
// v_mfma_f32_16x16x32_bf16, so the sums are those of skinny_mfma.hip over the
// dequantized weights.
//
// Work split, as skinny_mfma.hip: workgroup = 4 waves = 256 weight rows over
// one k-slice K/S, grid (ceil(N/256), S); a wave owns 64 rows as 4 row tiles;
// the waves share ONE staged x slice; token tiers MT = 16/32/64 with
// acc[4][MT/16] f32x4 in registers.  A wave whose rows start at or past N
// helps staging and leaves.
//
// Operands (lane = (lo, hi) = (lane & 15, lane >> 4)), per 128-k chunk c of 4
// scale blocks and row tile rt:
//   A: the lane loads ONE 16-byte unit, row n0 + 16*rt + lo, block 4*c + hi:
//      a whole scale block, 4 dwords of 8 nibbles.  Dword u is the lane's A
//      fragment of the chunk's MFMA u, so MFMA u multiplies, in k-slot
//      8*hi + j, the weights k = 128*c + 32*hi + 8*u + j.  The sum over a
//      chunk's 4 MFMAs covers its 128 k once; which k shares an MFMA is free
//      as long as B agrees.  A lane therefore fetches 4 k-steps in one wide
//      load, under ONE scale (its own: no lane shares a register's scale with
//      another row or block), and a wave's load instruction covers four
//      256-byte runs (16 rows x 16 bytes, one per hi).  Weights go global ->
//      registers -> MFMA, each byte loaded once per call.  The 8 scale bytes
//      of a row's 256 k are one 8-byte load per row tile.
//   B: x is staged so that B keeps the bf16 kernel's addresses: within every
//      128-k chunk the 16 groups of 8 k are transposed 4 x 4 on the way into
//      LDS (group 4*a + b goes to slot 4*b + a), so the ds_read_b128 at column
//      32*u + 8*hi of the chunk returns x[token][128*c + 32*hi + 8*u ..+8],
//      the k of A above.  Row stride RS = K/S + 16 elements, conflict-free
//      for these reads exactly as argued in skinny_mfma.hip; the staging
//      writes of 16 consecutive lanes still cover 64 consecutive dwords (the
//      transposition permutes them inside one 256-byte window).
//   C[m = 4*hi + reg][n = lo]: 4 consecutive output columns of token
//      16*tt + lo, one 16-byte fp32 (8-byte bf16) store.
//
// Pipeline: the k-slice is walked in blocks of 256 k = 2 chunks: 8 unit loads
// and 4 scale loads, 160 bytes a lane.  Two register blocks alternate; a
// block is refilled (for two blocks ahead) right after its MFMAs, and both
// are issued BEFORE x is staged, so a block's MFMAs wait with the other
// block's 12 loads still outstanding.  Nibbles arrive at a quarter of the
// bf16 byte rate per MFMA, so the same 8 wide loads cover 4x the k of the
// bf16 kernel's block and twice its MFMAs.  A slice may be 1, 2, 3, ...
// blocks (K/S is any multiple of 256): the loop runs while both refills
// exist, and the peeled tail of 1 to 3 blocks holds the only conditional
// refill.
//
// Split-K and epilogue as skinny_mfma.hip: S > 1 stores fp32 partials
// part[S, M, N] (valid rows only) for skinny_finalize_kernel; S = 1 adds bias
// and stores bf16 from the accumulators.  No scale touches the accumulators.
//
// Envelope as the bf16 kernel: N % 64 == 0, K % 256 == 0, S divides K/256,
// MT * (K/S + 16) * 2 <= SKINNY_MFMA_LDS_MAX.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950):
//   MT = 16: 113 VGPRs + 28 AGPRs, MT = 32: 123 + 44, MT = 64: 150 + 112;
//   no scratch, no static LDS (the x slice is dynamic, MT * (K/S + 16) * 2
//   bytes); 256 threads a workgroup, so one wave per SIMD has all of them.
#include "common.h"
#include "launchers.h"
#include "skinny_fp4.h"

#define SF_WAVES 4  // waves per workgroup, 64 weight rows each
#define SF_PAD 16   // LDS row padding, elements

// one pipeline block of one lane: 2 chunks x 4 row tiles of 16-byte units and
// the 4 row tiles' scale groups
struct Fp4Block {
  u32x4_t w[2][4];
  u32x2_t s[4];
};

// wl / sl: the lane's unit (row tile 0, block hi) and scale group in the
// slice's first pipeline block
__device__ __forceinline__ void load_block(Fp4Block& b, const u32x4_t* wl,
                                           const u32x2_t* sl, int64_t N,
                                           int blk) {
#pragma unroll
  for (int cc = 0; cc < 2; ++cc)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
      b.w[cc][rt] = wl[(int64_t)(blk * 8 + cc * 4) * N + rt * 16];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) b.s[rt] = sl[(int64_t)blk * N + rt * 16];
}

// acc += W block . x block^T; xr is the lane's LDS address (row lo, column
// 8*hi) in the block's first k-step
template <int MT>
__device__ __forceinline__ void mfma_block(const Fp4Block& w, const short* xr,
                                           int RS, int hi,
                                           f32x4 (&acc)[4][MT / 16]) {
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    float sf[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) sf[rt] = fp4_scale(w.s[rt][cc], hi);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bf16x8 b[MT / 16];
#pragma unroll
      for (int tt = 0; tt < MT / 16; ++tt)
        b[tt] = *reinterpret_cast<const bf16x8*>(xr + tt * 16 * RS +
                                                 (cc * 4 + u) * 32);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        bf16x8 a = __builtin_bit_cast(
            bf16x8, fp4x8_to_bf16(w.w[cc][rt][u], sf[rt]));
#pragma unroll
        for (int tt = 0; tt < MT / 16; ++tt)
          acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, b[tt], acc[rt][tt], 0, 0, 0);
      }
    }
  }
}

template <int MT>
__launch_bounds__(SF_WAVES * 64)
__global__ void skinny_mfma_fp4_kernel(
    const u32x4_t* __restrict__ wq,  // [K/32, N] blocks of 32 nibbles
    const u32x2_t* __restrict__ sq,  // [K/256, N] groups of 8 scale bytes
    const short* __restrict__ x,     // [M, K] bf16
    float* __restrict__ part,        // [S, M, N] fp32, or null when S == 1
    const short* __restrict__ bias,  // [N] or null (S == 1 only)
    short* __restrict__ y,           // [M, N] bf16 (S == 1 only)
    int M, int64_t N, int64_t K, int ksl) {
  extern __shared__ __attribute__((aligned(16))) short xs[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int RS = ksl + SF_PAD;
  const int64_t k0 = (int64_t)blockIdx.y * ksl;
  const int64_t n0 = ((int64_t)blockIdx.x * SF_WAVES + wave) * 64;
  const bool live = n0 < N;
  const int nblk = ksl >> 8;  // pipeline blocks of 256 k, >= 1

  // the first two blocks, in flight while x is staged (a wave with no rows
  // reads rows 0..63 and drops them; a one-block slice loads its block twice)
  const int64_t nl = (live ? n0 : 0) + lo;
  const u32x4_t* wl = wq + ((k0 >> 5) + hi) * N + nl;
  const u32x2_t* sl = sq + (k0 >> 8) * N + nl;
  Fp4Block wa, wb;
  load_block(wa, wl, sl, N, 0);
  load_block(wb, wl, sl, N, nblk > 1 ? 1 : 0);

  // MT * gpr groups of 16 bytes, gpr = ksl/8 a multiple of 32: gpr/32
  // rounds of XU = MT/8 independent loads per thread, no tail.  Group
  // 16*c + 4*a + b of a row is written to slot 16*c + 4*b + a.
  constexpr int XU = MT / 8;
  const int gpr = ksl >> 3;
  for (int i0 = threadIdx.x; i0 < MT * gpr; i0 += XU * SF_WAVES * 64) {
    bf16x8 v[XU];
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * SF_WAVES * 64;
      const int m = i / gpr, g = i - m * gpr;
      v[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (m < M)
        v[u] = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * K + k0 +
                                                g * 8);
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * SF_WAVES * 64;
      const int m = i / gpr, g = i - m * gpr;
      const int slot = (g & ~15) | ((g & 3) << 2) | ((g >> 2) & 3);
      *reinterpret_cast<bf16x8*>(xs + m * RS + slot * 8) = v[u];
    }
  }
  __syncthreads();
  if (!live) return;

  f32x4 acc[4][MT / 16];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int tt = 0; tt < MT / 16; ++tt) acc[rt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const short* xr = xs + lo * RS + hi * 8;
  // the loop runs while both refills exist; the barriers keep the written
  // order (the scheduler, left alone, sinks the refills to the loop's end)
  int blk = 0;
  for (; blk + 3 < nblk; blk += 2) {
    mfma_block<MT>(wa, xr + blk * 256, RS, hi, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_block(wa, wl, sl, N, blk + 2);
    __builtin_amdgcn_sched_barrier(0);
    mfma_block<MT>(wb, xr + (blk + 1) * 256, RS, hi, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_block(wb, wl, sl, N, blk + 3);
    __builtin_amdgcn_sched_barrier(0);
  }
  // 1, 2 or 3 blocks are left; wa holds the first, wb the second
  const int rem = nblk - blk;
  mfma_block<MT>(wa, xr + blk * 256, RS, hi, acc);
  if (rem == 3) load_block(wa, wl, sl, N, blk + 2);
  if (rem >= 2) mfma_block<MT>(wb, xr + (blk + 1) * 256, RS, hi, acc);
  if (rem == 3) mfma_block<MT>(wa, xr + (blk + 2) * 256, RS, hi, acc);

  // the lane's 4 x 4 output columns are the same for every token tile
  f32x4 bf[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    bf16x4 bv = {0, 0, 0, 0};
    if (bias)
      bv = *reinterpret_cast<const bf16x4*>(bias + n0 + rt * 16 + 4 * hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[rt][j] = bf2f(bv[j]);
  }
#pragma unroll
  for (int tt = 0; tt < MT / 16; ++tt) {
    const int token = tt * 16 + lo;
    if (token >= M) continue;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int64_t n = n0 + rt * 16 + 4 * hi;
      f32x4 v = acc[rt][tt];
      if (part) {
        *reinterpret_cast<f32x4*>(
            part + ((int64_t)blockIdx.y * M + token) * N + n) = v;
      } else {
        v += bf[rt];
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f2bf(v[j]);
        *reinterpret_cast<bf16x4*>(y + (int64_t)token * N + n) = o;
      }
    }
  }
}

extern "C" {

// part_or_null: fp32 [splits, M, N] when splits > 1, null when splits == 1.
// hipErrorInvalidValue outside the envelope (see launchers.h).
hipError_t launch_skinny_mfma_fp4(const void* wq, const void* sq,
                                  const void* x, float* part_or_null,
                                  const void* bias_or_null, void* y,
                                  int64_t M, int64_t N, int64_t K, int splits,
                                  hipStream_t stream) {
  if (M < 9 || M > 64 || N <= 0 || N % 64 || K <= 0 || K % 256 ||
      splits < 1 || (K / 256) % splits || (splits > 1) != (part_or_null != 0))
    return hipErrorInvalidValue;
  const int MT = M <= 16 ? 16 : M <= 32 ? 32 : 64;
  const int ksl = (int)(K / splits);
  const size_t lds = (size_t)MT * (ksl + SF_PAD) * sizeof(short);
  if (lds > SKINNY_MFMA_LDS_MAX) return hipErrorInvalidValue;
  dim3 grid((uint32_t)((N + SF_WAVES * 64 - 1) / (SF_WAVES * 64)),
            (uint32_t)splits);
  dim3 blk(SF_WAVES * 64);
  const void* bias_fused = splits == 1 ? bias_or_null : nullptr;
#define DISPATCH(MTC)                                                       \
  skinny_mfma_fp4_kernel<MTC><<<grid, blk, lds, stream>>>(                  \
      (const u32x4_t*)wq, (const u32x2_t*)sq, (const short*)x, part_or_null, \
      (const short*)bias_fused, (short*)y, (int)M, N, K, ksl)
  if (MT == 16) DISPATCH(16);
  else if (MT == 32) DISPATCH(32);
  else DISPATCH(64);
#undef DISPATCH
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || splits == 1) return err;
  const int64_t total = M * N;
  skinny_finalize_kernel<<<dim3((uint32_t)((total + 255) / 256)), dim3(256),
                           0, stream>>>(part_or_null,
                                        (const short*)bias_or_null, (short*)y,
                                        M, M, N, splits);
  return hipGetLastError();
}

}  // extern "C"
