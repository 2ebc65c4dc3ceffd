// MFMA skinny GEMM for gfx950: y[M,N] = x[M,K] @ W[N,K]^T (+ bias) for
// decode batches of 9 <= M <= 64 tokens, over the packed weights of the dot2
// kernel (skinny_gemm.hip): Wp[K/8][N][8], bf16 or e4m3 with one fp32 scale.
//
// Why a second kernel: the dot2 kernel gives every lane one weight row and
// MT accumulators, so its VALU work grows with M and it is issue-bound from
// M = 16.  Here one v_mfma_f32_16x16x32_bf16 does 16 weight rows x 16 tokens
// x 32 k, and the per-weight work outside the matrix unit (address, load,
// the e4m3 conversion) does not depend on M.
//
// Operands (lane = (lo, hi) = (lane & 15, lane >> 4)):
//   A = weights: A[m = lo][k = 8*hi + j] is row n0+lo of k-group k0/8 + hi,
//       ONE 16-byte load (8 bytes for e4m3) at ((k0/8+hi)*N + n0+lo)*8 --
//       the packed layout is already the A fragment.  A wave owns 64
//       consecutive rows as 4 row tiles, so its 4 loads of one k-step take
//       each k-group's contiguous 1-KB (512-B) segment completely.  Weights
//       go global -> registers -> MFMA, each byte loaded once per call.
//   B = tokens:  B[k = 8*hi + j][n = lo] is x[token 16*tt + lo][k0 + 8*hi + j],
//       a ds_read_b128 from the staged x slice; each fragment feeds the 4
//       row tiles' MFMAs.
//   C[m = 4*hi + reg][n = lo]: a lane ends with 4 consecutive output columns
//       of token 16*tt + lo -- one 16-byte fp32 (8-byte bf16) store.
// Token tiers MT = 16/32/64 are a template parameter: acc[4][MT/16] f32x4
// lives in registers (16/32/64 VGPRs).
//
// Workgroup = 4 waves = 256 weight rows; grid (ceil(N/256), S).  The waves
// share ONE staged x slice [MT, K/S]: against one wave per workgroup that
// cuts the x traffic from L2 and the LDS per wave to a quarter (at MT = 64 a
// 1-wave workgroup reads as many x bytes from L2 as weight bytes from HBM),
// and four independent load streams per workgroup hide HBM latency without
// more registers per wave.  Splitting the waves over k instead would need an
// LDS reduction of 64 x MT floats per wave.  A wave whose rows start at or
// past N (N % 256 != 0) helps staging and leaves.
//
// Pipeline: the k-slice is walked in blocks of KB = 2 k-steps (8 weight
// loads).  Two register blocks alternate; a block is refilled (for two
// blocks ahead) right after its MFMAs, and the first two blocks' loads are
// issued BEFORE x is staged, so the MFMAs of a block wait with the other
// block's 8 loads still outstanding behind them (the dot2 kernel's v1 -> v2
// lesson: one outstanding load runs at HBM latency, not bandwidth).  The x
// staging issues MT/8 independent 16-byte loads per thread before it writes.
//
// x slice in LDS: row stride RS = K/S + 16 elements.  K/S is a multiple of
// 256, so RS/2 = 8 (mod 16) dwords: a row is an odd multiple of 8 dwords.
// Rows at or past M are written as zeros and never read from memory, so the
// caller passes x unpadded.  By the bank rule (bank = dword mod 64), as for
// the row fragments of attention_bwd.hip:
//   - ds_read_b128 fragments (16 lanes on 16 rows, the 4 hi groups 16 bytes
//     apart): the 8 distinct rows mod 8 of a 16-lane group land on 8 distinct
//     8-dword slots, its two hi values on the two 4-dword halves of a slot --
//     64 banks, each once: conflict-free;
//   - the staging ds_write_b128 of consecutive lanes go to consecutive 16
//     bytes of a row (a row change moves on by 8 dwords) -- conflict-free.
// The slice is limited to SKINNY_MFMA_LDS_MAX bytes (the CU's 160 KB).
//
// Split-K: S > 1 stores fp32 partials part[S, M, N] (valid rows only, no
// zero fill, no atomics) and skinny_finalize_kernel reduces them in fixed
// order, adds bias and rounds.  S = 1 adds bias and stores bf16 straight
// from the accumulators: one launch.  e4m3 weights are converted to bf16 in
// registers (exact) and the scale is applied once to the fp32 result.
#include "common.h"
#include "launchers.h"

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// defined in skinny_gemm.hip; part is [splits, MT, N], rows 0..M-1 are read
__global__ void skinny_finalize_kernel(const float* __restrict__ part,
                                       const short* __restrict__ bias,
                                       short* __restrict__ y, int64_t MT,
                                       int64_t M, int64_t N, int splits);

#define SM_WAVES 4   // waves per workgroup, 64 weight rows each
#define SM_KB 2      // k-steps (of 32) per pipeline block
#define SM_PAD 16    // LDS row padding, elements

// one lane's weight fragment as loaded: 8 bf16 or 8 e4m3 bytes
template <bool FP8> struct WRaw { typedef bf16x8 T; };
template <> struct WRaw<true> { typedef u32x2_t T; };

__device__ __forceinline__ bf16x8 to_bf16(bf16x8 v) { return v; }

// e4m3 -> bf16 is exact, so the upper halves of the converted floats are
// the bf16 values
__device__ __forceinline__ bf16x8 to_bf16(u32x2_t v) {
  u32x4_t r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(v[h], false);
    f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8(v[h], true);
    r[2 * h] = (__float_as_uint(a[0]) >> 16) |
               (__float_as_uint(a[1]) & 0xffff0000u);
    r[2 * h + 1] = (__float_as_uint(b[0]) >> 16) |
                   (__float_as_uint(b[1]) & 0xffff0000u);
  }
  return __builtin_bit_cast(bf16x8, r);
}

// the 4 row tiles of SM_KB k-steps: p is the lane's address in the first
// k-step, kstep the byte distance between k-steps (4 k-groups)
template <bool FP8>
__device__ __forceinline__ void load_block(
    typename WRaw<FP8>::T (&w)[SM_KB][4], const char* p, int64_t kstep) {
  typedef typename WRaw<FP8>::T T;
#pragma unroll
  for (int u = 0; u < SM_KB; ++u)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
      w[u][rt] = *reinterpret_cast<const T*>(p + u * kstep +
                                             rt * 16 * (int)sizeof(T));
}

// acc += W block . x block^T; xr is the lane's LDS address (row lo, column
// 8*hi) in the block's first k-step
template <int MT, bool FP8>
__device__ __forceinline__ void mfma_block(
    const typename WRaw<FP8>::T (&w)[SM_KB][4], const short* xr, int RS,
    f32x4 (&acc)[4][MT / 16]) {
#pragma unroll
  for (int u = 0; u < SM_KB; ++u) {
    bf16x8 b[MT / 16];
#pragma unroll
    for (int tt = 0; tt < MT / 16; ++tt)
      b[tt] = *reinterpret_cast<const bf16x8*>(xr + tt * 16 * RS + u * 32);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      bf16x8 a = to_bf16(w[u][rt]);
#pragma unroll
      for (int tt = 0; tt < MT / 16; ++tt)
        acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, b[tt], acc[rt][tt], 0, 0, 0);
    }
  }
}

template <int MT, bool FP8>
__launch_bounds__(SM_WAVES * 64)
__global__ void skinny_mfma_kernel(
    const char* __restrict__ wp,       // [K/8, N, 8] packed bf16 / e4m3
    const short* __restrict__ x,       // [M, K] bf16
    float* __restrict__ part,          // [S, M, N] fp32, or null when S == 1
    const short* __restrict__ bias,    // [N] or null (S == 1 only)
    short* __restrict__ y,             // [M, N] bf16 (S == 1 only)
    const float* __restrict__ wscale,  // [1] (e4m3 only)
    int M, int64_t N, int64_t K, int ksl) {
  typedef typename WRaw<FP8>::T W;
  extern __shared__ __attribute__((aligned(16))) short xs[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int RS = ksl + SM_PAD;
  const int64_t k0 = (int64_t)blockIdx.y * ksl;
  const int64_t n0 = ((int64_t)blockIdx.x * SM_WAVES + wave) * 64;
  const bool live = n0 < N;

  // first weight block, in flight while x is staged (a wave with no rows
  // reads rows 0..63 and drops them)
  const int64_t kstep = 4 * N * (int64_t)sizeof(W);
  const char* wl = wp + (((k0 >> 3) + hi) * N + (live ? n0 : 0) + lo) *
                            (int64_t)sizeof(W);
  W wa[SM_KB][4], wb[SM_KB][4];
  load_block<FP8>(wa, wl, kstep);
  load_block<FP8>(wb, wl + SM_KB * kstep, kstep);

  // MT * gpr groups of 16 bytes, gpr = ksl/8 a multiple of 32: gpr/32
  // rounds of XU = MT/8 independent loads per thread, no tail
  constexpr int XU = MT / 8;
  const int gpr = ksl >> 3;
  for (int i0 = threadIdx.x; i0 < MT * gpr; i0 += XU * SM_WAVES * 64) {
    bf16x8 v[XU];
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * SM_WAVES * 64;
      const int m = i / gpr, g = i - m * gpr;
      v[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (m < M)
        v[u] = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * K + k0 +
                                                g * 8);
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * SM_WAVES * 64;
      const int m = i / gpr, g = i - m * gpr;
      *reinterpret_cast<bf16x8*>(xs + m * RS + g * 8) = v[u];
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
  const int nblk = ksl / (32 * SM_KB);  // a multiple of 4
  // the last two blocks are peeled: a refill under a condition would make
  // the waits behind it count for both paths, i.e. drain the new loads
  // (and the scheduler, left alone, sinks both refills to the loop's end,
  // below waits down to vmcnt(0): the barriers keep the written order)
  int blk = 0;
  for (; blk < nblk - 2; blk += 2) {
    mfma_block<MT, FP8>(wa, xr + blk * SM_KB * 32, RS, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_block<FP8>(wa, wl + (blk + 2) * SM_KB * kstep, kstep);
    __builtin_amdgcn_sched_barrier(0);
    mfma_block<MT, FP8>(wb, xr + (blk + 1) * SM_KB * 32, RS, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_block<FP8>(wb, wl + (blk + 3) * SM_KB * kstep, kstep);
    __builtin_amdgcn_sched_barrier(0);
  }
  mfma_block<MT, FP8>(wa, xr + blk * SM_KB * 32, RS, acc);
  mfma_block<MT, FP8>(wb, xr + (blk + 1) * SM_KB * 32, RS, acc);

  const float ws = FP8 ? *wscale : 1.f;
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
      f32x4 v = acc[rt][tt] * ws;
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

// part_or_null: fp32 [splits, M, N] when splits > 1, null when splits == 1;
// e4m3 weights iff wscale_or_null is given.  hipErrorInvalidValue outside
// the envelope (see launchers.h).
hipError_t launch_skinny_mfma(const void* wp, const void* x,
                              float* part_or_null, const void* bias_or_null,
                              void* y, const float* wscale_or_null,
                              int64_t M, int64_t N, int64_t K, int splits,
                              hipStream_t stream) {
  if (M < 9 || M > 64 || N <= 0 || N % 64 || K <= 0 || K % 256 ||
      splits < 1 || (K / 256) % splits || (splits > 1) != (part_or_null != 0))
    return hipErrorInvalidValue;
  const int MT = M <= 16 ? 16 : M <= 32 ? 32 : 64;
  const int ksl = (int)(K / splits);
  const size_t lds = (size_t)MT * (ksl + SM_PAD) * sizeof(short);
  if (lds > SKINNY_MFMA_LDS_MAX) return hipErrorInvalidValue;
  dim3 grid((uint32_t)((N + SM_WAVES * 64 - 1) / (SM_WAVES * 64)),
            (uint32_t)splits);
  dim3 blk(SM_WAVES * 64);
  const void* bias_fused = splits == 1 ? bias_or_null : nullptr;
#define DISPATCH(MTC)                                                      \
  do {                                                                     \
    if (wscale_or_null)                                                    \
      skinny_mfma_kernel<MTC, true><<<grid, blk, lds, stream>>>(           \
          (const char*)wp, (const short*)x, part_or_null,                  \
          (const short*)bias_fused, (short*)y, wscale_or_null, (int)M, N,  \
          K, ksl);                                                         \
    else                                                                   \
      skinny_mfma_kernel<MTC, false><<<grid, blk, lds, stream>>>(          \
          (const char*)wp, (const short*)x, part_or_null,                  \
          (const short*)bias_fused, (short*)y, nullptr, (int)M, N, K,      \
          ksl);                                                            \
  } while (0)
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
