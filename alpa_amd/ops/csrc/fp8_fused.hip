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

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------ bias + GeLU
// x [M, F] bf16, bias [F] -> q e4m3 [M, F], qt e4m3 [F, M]; no bf16 output.
// The tiling of fp8_quantize_dual_kernel: a 64x64 tile converted into LDS
// as fp8 bytes, then drained row-major and transposed, 16 B per lane.
#define FQT 64

__global__ void bias_gelu_fp8_kernel(const short* __restrict__ x,
                                     const short* __restrict__ bias,
                                     unsigned char* __restrict__ q,
                                     unsigned char* __restrict__ qt,
                                     const float* __restrict__ scale,
                                     float* __restrict__ amax_out,
                                     int64_t M, int64_t F) {
  const float inv = 1.0f / fmaxf(*scale, 1e-12f);
  __shared__ unsigned char tile[FQT][FQT + 4];  // +4 bytes: depivot banks
  const int64_t row0 = (int64_t)blockIdx.y * FQT;
  const int64_t col0 = (int64_t)blockIdx.x * FQT;
  const int t = threadIdx.x;           // 256 threads
  const int tc = (t & 15) * 4;         // 4 consecutive cols
  const int tr = t >> 4;               // 16 rows per pass
  const bool interior = (row0 + FQT <= M) && (col0 + FQT <= F);
  // 16-byte stores need 16-byte row pitches (F % 8 == 0 alone gives 8)
  const bool vec_q = interior && (F % 16 == 0);
  const bool vec_qt = interior && (M % 16 == 0);
  // F % 8 == 0 and tc % 4 == 0: a column quad is inside or outside whole
  const bool col_ok = col0 + tc < F;
  bf16x4 bv = {0, 0, 0, 0};
  if (col_ok) bv = *reinterpret_cast<const bf16x4*>(bias + col0 + tc);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = tr + i * 16;
    const int64_t gr = row0 + r;
    // outside the tensor: zeros, which neither move amax nor get stored
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (gr < M && col_ok) {
      bf16x4 v = *reinterpret_cast<const bf16x4*>(x + gr * F + col0 + tc);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        f[j] = bf2f(f2bf(gelu_f(bf2f(v[j]) + bf2f(bv[j]))));
    }
    unsigned char b[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned short p = cvt2_fp8<false>(f[2 * j] * inv, f[2 * j + 1] * inv);
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
  // row-major q, 16 B/lane (4 lanes cover one 64-B tile row)
  {
    const int r = t >> 2;               // 0..63 tile row
    const int c16 = (t & 3) * 16;
    const int64_t gr = row0 + r;
    if (vec_q) {
      u8x16 v;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[r][c16 + j];
      *reinterpret_cast<u8x16*>(q + gr * F + col0 + c16) = v;
    } else if (gr < M) {
      for (int j = 0; j < 16; ++j)
        if (col0 + c16 + j < F) q[gr * F + col0 + c16 + j] = tile[r][c16 + j];
    }
  }
  // transposed qt, 16 B/lane along the original row dim
  {
    const int r = t >> 2;               // 0..63 = original col = qt row
    const int c16 = (t & 3) * 16;       // original rows = qt cols
    const int64_t gq = col0 + r;
    if (vec_qt) {
      u8x16 v;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[c16 + j][r];
      *reinterpret_cast<u8x16*>(qt + gq * M + row0 + c16) = v;
    } else if (gq < F) {
      for (int j = 0; j < 16; ++j)
        if (row0 + c16 + j < M)
          qt[gq * M + row0 + c16 + j] = tile[c16 + j][r];
    }
  }
  __shared__ float red[16];
  amax = block_reduce_max(amax, red);
  if (threadIdx.x == 0) atomic_max_f32(amax_out, amax);
}

// ------------------------------------------------------- add + LayerNorm
// h = a + b (b may be null); y = LN(h) * w + bias is quantized, not stored.
//
// A workgroup walks FLN_ROWS consecutive rows, FLN_RI at a time, each with
// the row loop of add_layer_norm_fwd_kernel (h written, the two block
// reductions in the same order, statistics of the rounded h).  The
// normalize pass rounds y to bf16, casts it, stores q and parks the bytes
// in an LDS tile [16][H]; at the end the tile is drained into qt, 16 B
// along the row dimension per store.  16 * H bytes of LDS: H <= 4096.
// Consecutive row groups run on one XCD (xcd_swizzle), so the 16-B pieces
// of a qt line meet in one L2.
#define FLN_BLOCK 256
#define FLN_ROWS 16
#define FLN_RI 4
#define FLN_MAX_H 4096

// The compiler builds add_layer_norm_fwd_kernel's variance from separate
// multiplies and adds and its normalize step from fused multiply-adds.  A
// kernel that walks several rows at once is vectorized differently and
// would contract differently if left to the compiler, so both choices are
// spelled out here; the byte comparisons in the GPU tests hold them to
// what the one-row kernel does.
__device__ __forceinline__ float fln_sq_acc(float s, float d) {
#pragma clang fp contract(off)
  float p = d * d;
  return s + p;
}

// RI rows go through the three passes of add_layer_norm_fwd_kernel side by
// side: the loads of all RI rows are in flight together, each row keeps its
// own partial sums and its own block reductions, so every row's arithmetic
// is that of the one-row kernel.
template <int RI>
__device__ __forceinline__ void fln_rows(
    const short* __restrict__ a, const short* __restrict__ b,
    const short* __restrict__ w, const short* __restrict__ bias,
    short* __restrict__ h, unsigned char* __restrict__ q,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    unsigned char* tile_rows, float* red, int64_t row, int H, float eps,
    float inv, float& amax) {
  const short* ar = a + row * H;
  const short* br = (b == nullptr) ? nullptr : b + row * H;
  short* hr = h + row * H;
  float s[RI], mean[RI], rstd[RI];
#pragma unroll
  for (int u = 0; u < RI; ++u) s[u] = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += FLN_BLOCK * 8) {
    bf16x8 av[RI], bv[RI];
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      av[u] = *reinterpret_cast<const bf16x8*>(ar + (int64_t)u * H + i);
      if (br != nullptr)
        bv[u] = *reinterpret_cast<const bf16x8*>(br + (int64_t)u * H + i);
    }
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      bf16x8 hv;
      if (br != nullptr) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          hv[j] = f2bf(bf2f(av[u][j]) + bf2f(bv[u][j]));
          s[u] += bf2f(hv[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          hv[j] = av[u][j];
          s[u] += bf2f(av[u][j]);
        }
      }
      *reinterpret_cast<bf16x8*>(hr + (int64_t)u * H + i) = hv;
    }
  }
#pragma unroll
  for (int u = 0; u < RI; ++u) mean[u] = block_reduce_sum(s[u], red) / H;
  // two-pass variance; each thread re-reads the h elements it wrote itself
  // (here and in the normalize pass), so no fence is needed
#pragma unroll
  for (int u = 0; u < RI; ++u) s[u] = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += FLN_BLOCK * 8) {
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      bf16x8 hv = *reinterpret_cast<const bf16x8*>(hr + (int64_t)u * H + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = bf2f(hv[j]) - mean[u];
        s[u] = fln_sq_acc(s[u], d);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RI; ++u)
    rstd[u] = rsqrtf(block_reduce_sum(s[u], red) / H + eps);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      mean_out[row + u] = mean[u];
      rstd_out[row + u] = rstd[u];
    }
  }
  // normalize, round to bf16, cast; q goes out, the bytes are parked
  for (int i = threadIdx.x * 8; i < H; i += FLN_BLOCK * 8) {
    const bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + i);
    const bf16x8 bv2 = *reinterpret_cast<const bf16x8*>(bias + i);
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      bf16x8 hv = *reinterpret_cast<const bf16x8*>(hr + (int64_t)u * H + i);
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = (bf2f(hv[j]) - mean[u]) * rstd[u];
        f[j] = bf2f(f2bf(__builtin_fmaf(xhat, bf2f(wv[j]), bf2f(bv2[j]))));
        amax = fmaxf(amax, fabsf(f[j]));
      }
      u8x8 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned short p = cvt2_fp8<false>(f[2 * j] * inv, f[2 * j + 1] * inv);
        o[2 * j] = (unsigned char)(p & 0xff);
        o[2 * j + 1] = (unsigned char)(p >> 8);
      }
      *reinterpret_cast<u8x8*>(q + (row + u) * H + i) = o;
      *reinterpret_cast<u8x8*>(tile_rows + (int64_t)u * H + i) = o;
    }
  }
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
  const float inv = 1.0f / fmaxf(*scale, 1e-12f);
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
  dim3 grid((uint32_t)ceil_div(F, FQT), (uint32_t)ceil_div(M, FQT));
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
