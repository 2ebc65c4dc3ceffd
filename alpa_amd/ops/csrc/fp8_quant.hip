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
#include "fused_math.h"  // fp8_pack, fp8_quantize_tile, atomic_max_f32
#include "launchers.h"

// -------------------- single layout --------------------
// src bf16 [total], q fp8 [total]; q = src / *scale; amax_out = max|src|
template <bool E5M2>
__global__ void fp8_quantize_kernel(const short* __restrict__ src,
                                    unsigned char* __restrict__ q,
                                    const float* __restrict__ scale,
                                    float* __restrict__ amax_out,
                                    int64_t total) {
  const float inv = fp8_inv_scale(scale);
  float amax = 0.f;
  int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (; idx < total; idx += stride) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(src + idx);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
    u8x8 o;
    fp8_pack<E5M2, 4>(f, inv, amax, o);
    *reinterpret_cast<u8x8*>(q + idx) = o;
  }
  __shared__ float red[16];
  amax = block_reduce_max(amax, red);
  if (threadIdx.x == 0) atomic_max_f32(amax_out, amax);
}

// -------------------- dual layout --------------------
// src bf16 [M, N] -> q fp8 [M, N] AND qT fp8 [N, M], one read of src.
// The 64x64 tile routine of fused_math.h with a loader that reads src.
template <bool E5M2>
__global__ void fp8_quantize_dual_kernel(const short* __restrict__ src,
                                         unsigned char* __restrict__ q,
                                         unsigned char* __restrict__ qt,
                                         const float* __restrict__ scale,
                                         float* __restrict__ amax_out,
                                         int64_t M, int64_t N) {
  fp8_quantize_tile<E5M2>(
      [&](int64_t gr, int64_t gc) {
        f32x4 f = {0.f, 0.f, 0.f, 0.f};
        if (gr < M) {
          if (gc + 3 < N) {
            bf16x4 v = *reinterpret_cast<const bf16x4*>(src + gr * N + gc);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = bf2f(v[j]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (gc + j < N) f[j] = bf2f(src[gr * N + gc + j]);
          }
        }
        return f;
      },
      q, qt, scale, amax_out, M, N);
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
  dim3 grid((uint32_t)ceil_div(N, FP8_TILE), (uint32_t)ceil_div(M, FP8_TILE));
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
