// MFMA layout probes: one-wave kernels that run a single MFMA tile so the
// fragment layouts the attention kernels rely on (attention.hip header) can
// be verified against a CPU reference on real hardware.
#include "common.h"
#include "launchers.h"

// 16x16x32 layout probe: D(16x16) = A(16x32) @ B(32x16).
__global__ void mfma_probe_kernel(const short* __restrict__ a,
                                  const short* __restrict__ b,
                                  float* __restrict__ d) {
  int lane = threadIdx.x & 63;
  int lo = lane & 15, hi = lane >> 4;
  bf16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = a[lo * 32 + hi * 8 + j];       // A[m][k] row-major 16x32
    bf[j] = b[(hi * 8 + j) * 16 + lo];     // B[k][n] row-major 32x16
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) d[(hi * 4 + r) * 16 + lo] = acc[r];
}

extern "C" hipError_t launch_mfma_probe(const void* a, const void* b,
                                        float* d, hipStream_t stream) {
  mfma_probe_kernel<<<dim3(1), dim3(64), 0, stream>>>((const short*)a,
                                                      (const short*)b, d);
  return hipGetLastError();
}

// 32x32x16 layout probe: D(32x32) = A(32x16) @ B(16x32).
// Assumed layouts: A: m=lane&31, k=(lane>>5)*8+j; B: n=lane&31, same k;
// C/D (documented, guide §3): col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5)
__global__ void mfma_probe32_kernel(const short* __restrict__ a,
                                    const short* __restrict__ b,
                                    float* __restrict__ d) {
  int lane = threadIdx.x & 63;
  int lo = lane & 31, hi = lane >> 5;
  bf16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = a[lo * 16 + hi * 8 + j];
    bf[j] = b[(hi * 8 + j) * 32 + lo];
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
    d[row * 32 + lo] = acc[r];
  }
}

extern "C" hipError_t launch_mfma_probe32(const void* a, const void* b,
                                          float* d, hipStream_t stream) {
  mfma_probe32_kernel<<<dim3(1), dim3(64), 0, stream>>>((const short*)a,
                                                        (const short*)b, d);
  return hipGetLastError();
}
