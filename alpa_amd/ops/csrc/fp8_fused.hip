// fp8 (e4m3) quantization fused into the two forward kernels whose output
// only ever feeds an fp8 GEMM (gfx950).
//
// With the fp8 weight-grad GEMM on, the bf16 output of add+LayerNorm
// (qkv / fc1 input) and of bias+GeLU (fc2 input) is written once and read
// once — by the dual quantize.  These kernels emit the GEMM operands
// (q row-major, qt transposed, amax) straight from the producer, so the
// bf16 tensor never reaches HBM: 8 instead of 12 bytes per element for
// the LayerNorm pair, 4 instead of 8 for the GeLU pair.
//
// Bit-exactness: every value is computed in fp32 exactly as the unfused
// kernel does, rounded to bf16 with f2bf, and amax / the fp8 cast are
// taken from that rounded value with the same inv = 1/max(*scale, 1e-12).
// q, qt, amax (and h, mean, rstd) are byte-for-byte what
// add_layer_norm_fwd / bias_gelu_fwd followed by the dual quantize give.
#include "common.h"
#include "fused_math.h"
#include "launchers.h"
#include "layernorm_rows.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------ bias + GeLU
// x [M, F] bf16, bias [F] -> q e4m3 [M, F], qt e4m3 [F, M]; no bf16 output.
// The tile routine of fp8_quantize_dual_kernel (fused_math.h) with a loader
// that computes the bf16 rounding of gelu(x + bias) instead of reading it.
__global__ void bias_gelu_fp8_kernel(const short* __restrict__ x,
                                     const short* __restrict__ bias,
                                     unsigned char* __restrict__ q,
                                     unsigned char* __restrict__ qt,
                                     const float* __restrict__ scale,
                                     float* __restrict__ amax_out,
                                     int64_t M, int64_t F) {
  fp8_quantize_tile<false>(
      [&](int64_t gr, int64_t gc) {
        f32x4 f = {0.f, 0.f, 0.f, 0.f};
        // F % 8 == 0 and gc % 4 == 0: a column quad is inside or outside whole
        if (gr < M && gc < F) {
          bf16x4 v = *reinterpret_cast<const bf16x4*>(x + gr * F + gc);
          // re-loaded for each of a thread's four rows, on purpose: the
          // quad stays in L1, and the loader stays a function of (row, col)
          bf16x4 bv = *reinterpret_cast<const bf16x4*>(bias + gc);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            f[j] = bf2f(f2bf(gelu_f(bf2f(v[j]) + bf2f(bv[j]))));
        }
        return f;
      },
      q, qt, scale, amax_out, M, F);
}

// ------------------------------------------------------- add + LayerNorm
// h = a + b (b may be null); y = LN(h) * w + bias is quantized, not stored.
//
// A workgroup walks FLN_ROWS consecutive rows, FLN_RI at a time, through
// layer_norm_rows, the row passes add_layer_norm_fwd_kernel runs: h, mean,
// rstd and the bf16 rounding of y are that kernel's by construction.  The
// epilogue casts the rounded y, stores q and parks the bytes in an LDS tile
// [16][H]; at the end the tile is drained into qt, 16 B along the row
// dimension per store.  16 * H bytes of LDS: H <= 4096.
// Consecutive row groups run on one XCD (xcd_swizzle), so the 16-B pieces
// of a qt line meet in one L2.
#define FLN_BLOCK LN_BLOCK
#define FLN_ROWS 16
#define FLN_RI 4
#define FLN_MAX_H 4096

// RI rows from `row` on: q goes out, the bytes are parked in tile_rows
template <int RI>
__device__ __forceinline__ void fln_rows(
    const short* __restrict__ a, const short* __restrict__ b,
    const short* __restrict__ w, const short* __restrict__ bias,
    short* __restrict__ h, unsigned char* __restrict__ q,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    unsigned char* tile_rows, float* red, int64_t row, int H, float eps,
    float inv, float& amax) {
  layer_norm_rows<RI, true>(
      a, b, w, bias, h, mean_out, rstd_out, red, row, H, eps,
      [&](int u, int i, bf16x8 y) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = bf2f(y[j]);
        u8x8 o;
        fp8_pack<false, 4>(f, inv, amax, o);
        *reinterpret_cast<u8x8*>(q + (row + u) * H + i) = o;
        *reinterpret_cast<u8x8*>(tile_rows + (int64_t)u * H + i) = o;
      });
}

template <int RI>
__global__ void __launch_bounds__(FLN_BLOCK)
add_layer_norm_fp8_kernel(const short* __restrict__ a,
                               const short* __restrict__ b,
                               const short* __restrict__ w,
                               const short* __restrict__ bias,
                               short* __restrict__ h,
                               unsigned char* __restrict__ q,
                               unsigned char* __restrict__ qt,
                               float* __restrict__ mean_out,
                               float* __restrict__ rstd_out,
                               const float* __restrict__ scale,
                               float* __restrict__ amax_out, int64_t N,
                               int H, float eps) {
  // tile[FLN_ROWS][H] fp8 bytes and nothing else: at H = 2560 four
  // workgroups fill a CU's 160 KB exactly.  The reduction scratch lives in
  // the LAST tile row: every reduction of a row group ends (with a
  // barrier) before that group parks its bytes, and row 15 parks last.
  extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
  float* red = reinterpret_cast<float*>(tile + (FLN_ROWS - 1) * H);
  const float inv = fp8_inv_scale(scale);
  const int64_t row0 =
      (int64_t)xcd_swizzle((int)blockIdx.x, (int)gridDim.x) * FLN_ROWS;
  const int nrows = (int)min((int64_t)FLN_ROWS, N - row0);
  float amax = 0.f;
  int r = 0;
  for (; r + RI <= nrows; r += RI)
    fln_rows<RI>(a, b, w, bias, h, q, mean_out, rstd_out,
                 tile + (int64_t)r * H, red, row0 + r, H, eps, inv, amax);
  for (; r < nrows; ++r)
    fln_rows<1>(a, b, w, bias, h, q, mean_out, rstd_out,
                tile + (int64_t)r * H, red, row0 + r, H, eps, inv, amax);
  __syncthreads();
  // drain qt: a lane takes four columns of all 16 rows as dwords,
  // transposes them in registers and stores 16 B along the row dimension
  const bool vec_qt = (nrows == FLN_ROWS) && (N % 16 == 0);
  for (int col = threadIdx.x * 4; col < H; col += FLN_BLOCK * 4) {
    if (vec_qt) {
      unsigned int d[FLN_ROWS];
#pragma unroll
      for (int k = 0; k < FLN_ROWS; ++k)
        d[k] = *reinterpret_cast<const unsigned int*>(tile + k * H + col);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          o[k] = ((d[4 * k] >> (8 * j)) & 0xffu) |
                 (((d[4 * k + 1] >> (8 * j)) & 0xffu) << 8) |
                 (((d[4 * k + 2] >> (8 * j)) & 0xffu) << 16) |
                 (((d[4 * k + 3] >> (8 * j)) & 0xffu) << 24);
        *reinterpret_cast<u32x4*>(qt + (int64_t)(col + j) * N + row0) = o;
      }
    } else {
      for (int k = 0; k < nrows; ++k)
        for (int j = 0; j < 4; ++j)
          qt[(int64_t)(col + j) * N + row0 + k] = tile[k * H + col + j];
    }
  }
  __syncthreads();  // the tile is read out: its last row is scratch again
  amax = block_reduce_max(amax, red);
  if (threadIdx.x == 0) atomic_max_f32(amax_out, amax);
}

extern "C" {

hipError_t launch_bias_gelu_fp8(const void* x, const void* bias, void* q,
                                void* qt, const float* scale, float* amax,
                                int64_t M, int64_t F, hipStream_t stream) {
  dim3 grid((uint32_t)ceil_div(F, FP8_TILE), (uint32_t)ceil_div(M, FP8_TILE));
  bias_gelu_fp8_kernel<<<grid, dim3(256), 0, stream>>>(
      (const short*)x, (const short*)bias, (unsigned char*)q,
      (unsigned char*)qt, scale, amax, M, F);
  return hipGetLastError();
}

hipError_t launch_add_layer_norm_fp8(const void* a, const void* b,
                                     const void* w, const void* bias, void* h,
                                     void* q, void* qt, float* mean,
                                     float* rstd, const float* scale,
                                     float* amax, int64_t N, int64_t H,
                                     float eps, hipStream_t stream) {
  if (H > FLN_MAX_H) return hipErrorInvalidValue;
  dim3 grid((uint32_t)ceil_div(N, FLN_ROWS));
  // the tile, or 15 rows of it plus the reduction scratch when H < 16
  const size_t lds =
      (size_t)max((int64_t)FLN_ROWS * H, (FLN_ROWS - 1) * H + 16);
  add_layer_norm_fp8_kernel<FLN_RI>
      <<<grid, dim3(FLN_BLOCK), lds, stream>>>(
          (const short*)a, (const short*)b, (const short*)w,
          (const short*)bias, (short*)h, (unsigned char*)q,
          (unsigned char*)qt, mean, rstd, scale, amax, N, (int)H, eps);
  return hipGetLastError();
}

}  // extern "C"
