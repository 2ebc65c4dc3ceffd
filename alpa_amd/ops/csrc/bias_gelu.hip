// Fused bias + GeLU(tanh) forward/backward, bf16 (gfx950).
//
// The epilogue of the MLP up-projection GEMM (reference gets this from XLA
// fusion; SURVEY.md §2.3 N13 "GEMM+bias+GeLU epilogue").  Memory-bound:
// bf16x8 vector loads; dbias via deterministic striped partials, summed by
// colsum_finalize_kernel.
#include "common.h"
#include "fused_math.h"  // gelu_sigmoid, gelu_f
#include "launchers.h"

// d/dx of x * sigmoid(2z):  sg + 2x sg (1 - sg) k (1 + 3c x^2)
// (t = 2*sg - 1;  1 - t^2 = 4*sg*(1-sg)).  The two fused multiply-adds are
// spelled out and nothing else may contract: left to the compiler, the
// choice depends on how the caller's loop gets vectorized (one row or two
// side by side came out differently), and dx would change with the kernel's
// shape.  This is the form the flat dx kernel always computed.
__device__ __forceinline__ float gelu_grad_f(float x) {
  const float k = 0.7978845608028654f;
  float sg = gelu_sigmoid(x);
  {
#pragma clang fp contract(off)
    float a = 2.0f * x * sg * (1.0f - sg) * k;
    float p = __builtin_fmaf(x * x, 3.f * 0.044715f, 1.0f);
    return __builtin_fmaf(p, a, sg);
  }
}

// x [N, F] bf16, bias [F] -> y [N, F]
__global__ void bias_gelu_fwd_kernel(const short* __restrict__ x,
                                     const short* __restrict__ bias,
                                     short* __restrict__ y, int64_t total,
                                     int F) {
  int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (; idx < total; idx += stride) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(x + idx);
    bf16x8 bv = *reinterpret_cast<const bf16x8*>(bias + (idx % F));
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(gelu_f(bf2f(v[j]) + bf2f(bv[j])));
    *reinterpret_cast<bf16x8*>(y + idx) = o;
  }
}

// Backward in one pass, tiled like the column-sum partial below: block
// (c, p) owns 2048 columns and row stripe p, each thread 8 columns.  Per row
// a thread writes the bf16 dx and adds that ROUNDED dx (what the fc1 dW GEMM
// consumes) into its 8 fp32 column sums, rows in order, so db_part [P, F] is
// what bias_grad_partial_kernel gives for the stored dx, bit for bit.
#define BGB_ROWS 2  // rows in flight per thread: 4 independent 16-byte loads

__device__ __forceinline__ void bias_gelu_bwd_row(bf16x8 dv, bf16x8 xv,
                                                  bf16x8 bv, short* dxp,
                                                  float* s) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float z = bf2f(xv[j]) + bf2f(bv[j]);
    o[j] = f2bf(bf2f(dv[j]) * gelu_grad_f(z));
    s[j] += bf2f(o[j]);
  }
  *reinterpret_cast<bf16x8*>(dxp) = o;
}

__global__ void __launch_bounds__(256)
bias_gelu_bwd_kernel(const short* __restrict__ dy, const short* __restrict__ x,
                     const short* __restrict__ bias, short* __restrict__ dx,
                     float* __restrict__ db_part, int64_t N, int F) {
  const int col8 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const int p = blockIdx.y;
  const int P = gridDim.y;
  const int64_t r0 = (int64_t)p * N / P, r1 = (int64_t)(p + 1) * N / P;
  if (col8 + 8 <= F) {
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bias + col8);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t row = r0;
    for (; row + BGB_ROWS <= r1; row += BGB_ROWS) {
      bf16x8 dv[BGB_ROWS], xv[BGB_ROWS];
#pragma unroll
      for (int u = 0; u < BGB_ROWS; ++u) {
        dv[u] = *reinterpret_cast<const bf16x8*>(dy + (row + u) * F + col8);
        xv[u] = *reinterpret_cast<const bf16x8*>(x + (row + u) * F + col8);
      }
#pragma unroll
      for (int u = 0; u < BGB_ROWS; ++u)
        bias_gelu_bwd_row(dv[u], xv[u], bv, dx + (row + u) * F + col8, s);
    }
    for (; row < r1; ++row) {
      bf16x8 dv = *reinterpret_cast<const bf16x8*>(dy + row * F + col8);
      bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + row * F + col8);
      bias_gelu_bwd_row(dv, xv, bv, dx + row * F + col8, s);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) db_part[(int64_t)p * F + col8 + j] = s[j];
  } else if (col8 < F) {
    // a width that is no multiple of 8: its last columns, one at a time
    for (int c = col8; c < F; ++c) {
      const float b = bf2f(bias[c]);
      float s = 0.f;
      for (int64_t row = r0; row < r1; ++row) {
        short o = f2bf(bf2f(dy[row * F + c]) *
                       gelu_grad_f(bf2f(x[row * F + c]) + b));
        dx[row * F + c] = o;
        s += bf2f(o);
      }
      db_part[(int64_t)p * F + c] = s;
    }
  }
}

// column-sum partials (colsum_bf16, the bias grad of plain +bias layers):
// stripe p sums its row range of dx over an 8-column group per thread
// (bf16x8 loads — the scalar version was issue-bound at ~6x off the HBM
// roofline).
__global__ void bias_grad_partial_kernel(const short* __restrict__ dx,
                                         float* __restrict__ part, int64_t N,
                                         int F) {
  const int col8 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const int p = blockIdx.y;
  const int P = gridDim.y;
  const int64_t r0 = (int64_t)p * N / P, r1 = (int64_t)(p + 1) * N / P;
  if (col8 + 8 <= F) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t row = r0; row < r1; ++row) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(dx + row * F + col8);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += bf2f(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(int64_t)p * F + col8 + j] = s[j];
  } else if (col8 < F) {
    for (int c = col8; c < F; ++c) {
      float s = 0.f;
      for (int64_t row = r0; row < r1; ++row) s += bf2f(dx[row * F + c]);
      part[(int64_t)p * F + c] = s;
    }
  }
}

// The stripe sum behind every column reduction (dbias, LayerNorm dw/db):
// out[c] = sum over p of part[p, c], in the requested dtype.  A block owns
// FIN_COLS columns; 8 threads cover them with one 16-byte load per stripe
// row, FIN_SLICES such groups take the rows p = s, s + FIN_SLICES, ... and
// one thread per column adds the slice sums in slice order.  The order is a
// function of P alone, and the bf16 result is the fp32 one rounded to
// nearest even.  blockIdx.y picks the (part, out) pair: LayerNorm's dw and
// db go in one launch.
#define FIN_COLS 32
#define FIN_SLICES 32

__global__ void __launch_bounds__(FIN_COLS / 4 * FIN_SLICES)
colsum_finalize_kernel(const float* __restrict__ part_a,
                       const float* __restrict__ part_b, void* out_a,
                       void* out_b, int P, int F, int out_bf16) {
  const float* part = blockIdx.y == 0 ? part_a : part_b;
  void* out = blockIdx.y == 0 ? out_a : out_b;
  __shared__ float acc[FIN_SLICES][FIN_COLS];
  const int quad = threadIdx.x % (FIN_COLS / 4);
  const int slice = threadIdx.x / (FIN_COLS / 4);
  const int c0 = blockIdx.x * FIN_COLS + quad * 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (F % 4 == 0) {
    if (c0 < F) {
#pragma unroll 8
      for (int p = slice; p < P; p += FIN_SLICES) {
        f32x4 t = *reinterpret_cast<const f32x4*>(part + (int64_t)p * F + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += t[k];
      }
    }
  } else {
    // rows of such a width are not 16-byte aligned
    for (int p = slice; p < P; p += FIN_SLICES) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < F) v[k] += part[(int64_t)p * F + c0 + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[slice][quad * 4 + k] = v[k];
  __syncthreads();
  const int c = blockIdx.x * FIN_COLS + threadIdx.x;
  if (threadIdx.x < FIN_COLS && c < F) {
    float r = 0.f;
#pragma unroll
    for (int s = 0; s < FIN_SLICES; ++s) r += acc[s][threadIdx.x];
    if (out_bf16)
      reinterpret_cast<short*>(out)[c] = f2bf(r);
    else
      reinterpret_cast<float*>(out)[c] = r;
  }
}

extern "C" {

hipError_t launch_colsum_finalize(const float* part_a, const float* part_b,
                                  void* out_a, void* out_b, int P, int64_t F,
                                  int out_bf16, hipStream_t stream) {
  dim3 grid((uint32_t)ceil_div(F, FIN_COLS), part_b != nullptr ? 2 : 1);
  colsum_finalize_kernel<<<grid, dim3(FIN_COLS / 4 * FIN_SLICES), 0,
                           stream>>>(part_a, part_b, out_a, out_b, P, (int)F,
                                     out_bf16);
  return hipGetLastError();
}

hipError_t launch_bias_gelu_fwd(const void* x, const void* bias, void* y,
                                int64_t N, int64_t F, hipStream_t stream) {
  int64_t total = N * F;
  int blocks = (int)min((int64_t)2048, ceil_div(total, 256 * 8));
  bias_gelu_fwd_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(
      (const short*)x, (const short*)bias, (short*)y, total, (int)F);
  return hipGetLastError();
}

hipError_t launch_colsum_partial(const void* t, float* part, int64_t N,
                                 int64_t F, int P, hipStream_t stream) {
  dim3 grid((uint32_t)ceil_div(F, 256 * 8), P);
  bias_grad_partial_kernel<<<grid, dim3(256), 0, stream>>>(
      (const short*)t, part, N, (int)F);
  return hipGetLastError();
}

hipError_t launch_bias_gelu_bwd(const void* dy, const void* x,
                                const void* bias, void* dx, float* db_part,
                                int64_t N, int64_t F, int P,
                                hipStream_t stream) {
  dim3 grid((uint32_t)ceil_div(F, 256 * 8), P);
  bias_gelu_bwd_kernel<<<grid, dim3(256), 0, stream>>>(
      (const short*)dy, (const short*)x, (const short*)bias, (short*)dx,
      db_part, N, (int)F);
  return hipGetLastError();
}

}  // extern "C"
