// fp8 (OCP e4m3 / e5m2) quantization kernels for gfx950.
//
// The linchpin of the fp8 GEMM recipe: round-1 measured the torch-op
// cast path at up to 7.5 ms per tensor where the bandwidth bound is
// ~0.6 ms (profiles/fp8_bench).  These kernels do amax + scaled cast in
// ONE pass over HBM, and the dual variant additionally emits the
// TRANSPOSED fp8 copy through an LDS tile so the dW GEMM
// (dW = dY^T @ X) gets its row-major A operand without a second pass.
//
// Scaling is DELAYED: `scale` is read from a device pointer computed
// from the running amax of previous steps (no host sync, hipGraph-safe)
// while the CURRENT amax is reduced into `amax_out` via atomicMax on
// positive-float bits.
#include "common.h"
#include "fused_math.h"  // cvt2_fp8, atomic_max_f32, u8x8/u8x16
#include "launchers.h"

// -------------------- single layout --------------------
// src bf16 [total], q fp8 [total]; q = src / *scale; amax_out = max|src|
template <bool E5M2>
__global__ void fp8_quantize_kernel(const short* __restrict__ src,
                                    unsigned char* __restrict__ q,
                                    const float* __restrict__ scale,
                                    float* __restrict__ amax_out,
                                    int64_t total) {
  const float inv = 1.0f / fmaxf(*scale, 1e-12f);
  float amax = 0.f;
  int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (; idx < total; idx += stride) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(src + idx);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = bf2f(v[j]);
      amax = fmaxf(amax, fabsf(f[j]));
    }
    u8x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned short p = cvt2_fp8<E5M2>(f[2 * j] * inv, f[2 * j + 1] * inv);
      o[2 * j] = (unsigned char)(p & 0xff);
      o[2 * j + 1] = (unsigned char)(p >> 8);
    }
    *reinterpret_cast<u8x8*>(q + idx) = o;
  }
  __shared__ float red[16];
  amax = block_reduce_max(amax, red);
  if (threadIdx.x == 0) atomic_max_f32(amax_out, amax);
}

// -------------------- dual layout --------------------
// src bf16 [M, N] -> q fp8 [M, N] AND qT fp8 [N, M], one read of src.
// 64x64 tiles staged through LDS as already-converted fp8 bytes.
#define QT 64

template <bool E5M2>
__global__ void fp8_quantize_dual_kernel(const short* __restrict__ src,
                                         unsigned char* __restrict__ q,
                                         unsigned char* __restrict__ qt,
                                         const float* __restrict__ scale,
                                         float* __restrict__ amax_out,
                                         int64_t M, int64_t N) {
  // Phase 1 converts a 64x64 tile into LDS; phases 2/3 drain it with
  // 16-BYTE stores per lane (row-major q and transposed qt) so both
  // global write streams are fully coalesced — the first cut used
  // 4-byte scattered stores and ran 4x off the bandwidth roofline
  // (profiles/prof_fp8 r2).
  const float inv = 1.0f / fmaxf(*scale, 1e-12f);
  __shared__ unsigned char tile[QT][QT + 4];  // +4 bytes: depivot banks
  const int64_t row0 = (int64_t)blockIdx.y * QT;
  const int64_t col0 = (int64_t)blockIdx.x * QT;
  const int t = threadIdx.x;           // 256 threads
  const int tc = (t & 15) * 4;         // 4 consecutive cols
  const int tr = t >> 4;               // 16 rows per pass
  const bool interior =
      (row0 + QT <= M) && (col0 + QT <= N);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = tr + i * 16;
    const int64_t gr = row0 + r;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (gr < M) {
      if (col0 + tc + 3 < N) {
        bf16x4 v = *reinterpret_cast<const bf16x4*>(src + gr * N + col0 + tc);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = bf2f(v[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col0 + tc + j < N) f[j] = bf2f(src[gr * N + col0 + tc + j]);
      }
    }
    unsigned char b[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned short p =
          cvt2_fp8<E5M2>(f[2 * j] * inv, f[2 * j + 1] * inv);
      b[2 * j] = (unsigned char)(p & 0xff);
      b[2 * j + 1] = (unsigned char)(p >> 8);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      amax = fmaxf(amax, fabsf(f[j]));
      tile[r][tc + j] = b[j];
    }
  }
  __syncthreads();
  // phase 2: row-major q, 16 B/lane (4 lanes cover one 64-B tile row)
  {
    const int r = t >> 2;               // 0..63 tile row
    const int c16 = (t & 3) * 16;
    const int64_t gr = row0 + r;
    if (interior) {
      u8x16 v;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[r][c16 + j];
      *reinterpret_cast<u8x16*>(q + gr * N + col0 + c16) = v;
    } else if (gr < M) {
      for (int j = 0; j < 16; ++j)
        if (col0 + c16 + j < N) q[gr * N + col0 + c16 + j] = tile[r][c16 + j];
    }
  }
  // phase 3: transposed qt, 16 B/lane along the original row dim
  {
    const int r = t >> 2;               // 0..63 = original col = qt row
    const int c16 = (t & 3) * 16;       // original rows = qt cols
    const int64_t gq = col0 + r;
    if (interior) {
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

extern "C" {

hipError_t launch_fp8_quantize(const void* src, void* q, const float* scale,
                               float* amax, int64_t total, int e5m2,
                               hipStream_t stream) {
  int blocks = (int)min((int64_t)4096, ceil_div(total, 256 * 8));
  if (e5m2)
    fp8_quantize_kernel<true><<<dim3(blocks), dim3(256), 0, stream>>>(
        (const short*)src, (unsigned char*)q, scale, amax, total);
  else
    fp8_quantize_kernel<false><<<dim3(blocks), dim3(256), 0, stream>>>(
        (const short*)src, (unsigned char*)q, scale, amax, total);
  return hipGetLastError();
}

hipError_t launch_fp8_quantize_dual(const void* src, void* q, void* qt,
                                    const float* scale, float* amax,
                                    int64_t M, int64_t N, int e5m2,
                                    hipStream_t stream) {
  dim3 grid((uint32_t)ceil_div(N, QT), (uint32_t)ceil_div(M, QT));
  if (e5m2)
    fp8_quantize_dual_kernel<true><<<grid, dim3(256), 0, stream>>>(
        (const short*)src, (unsigned char*)q, (unsigned char*)qt, scale,
        amax, M, N);
  else
    fp8_quantize_dual_kernel<false><<<grid, dim3(256), 0, stream>>>(
        (const short*)src, (unsigned char*)q, (unsigned char*)qt, scale,
        amax, M, N);
  return hipGetLastError();
}

}  // extern "C"
