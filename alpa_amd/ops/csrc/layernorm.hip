// LayerNorm forward/backward for bf16 rows (gfx950).
//
// Memory-bound: target HBM ceiling via bf16x8 vector loads (guide G13),
// fp32 accumulation, one workgroup per row (fwd) or per stripe of rows (bwd),
// striped column-partial reduction for dw/db (deterministic — no atomics, so
// TP replicas stay bitwise identical).
//
// Covers the reference's LayerNorm fwd/bwd fusion slot (SURVEY.md §2.3
// kernel table: "LayerNorm fwd/bwd | elementwise+reduce fusion | [B·S, H]").
#include "common.h"
#include "launchers.h"
#include "layernorm_rows.h"

// ---------------------------------------------------------------- forward
// x [N, H] bf16, w/b [H] bf16 -> y [N, H] bf16, mean/rstd [N] fp32.
// One workgroup per row; the passes are layer_norm_rows (layernorm_rows.h).
__global__ void layer_norm_fwd_kernel(const short* __restrict__ x,
                                      const short* __restrict__ w,
                                      const short* __restrict__ b,
                                      short* __restrict__ y,
                                      float* __restrict__ mean_out,
                                      float* __restrict__ rstd_out,
                                      int H, float eps) {
  __shared__ float red[LN_BLOCK / 64];
  const int row = blockIdx.x;
  short* yr = y + (int64_t)row * H;
  layer_norm_rows<1, false>(
      x, nullptr, w, b, nullptr, mean_out, rstd_out, red, row, H, eps,
      [&](int, int i, bf16x8 o) { *reinterpret_cast<bf16x8*>(yr + i) = o; });
}

// Fused residual-add + LayerNorm: h = a + b; y = LN(h) * w + bias.
// Saves the separate elementwise-add pass over the residual stream
// (the reference gets this from XLA fusion).  b may be null (plain LN
// with h written = a, used at the embedding boundary).
__global__ void add_layer_norm_fwd_kernel(const short* __restrict__ a,
                                          const short* __restrict__ b,
                                          const short* __restrict__ w,
                                          const short* __restrict__ bias,
                                          short* __restrict__ h,
                                          short* __restrict__ y,
                                          float* __restrict__ mean_out,
                                          float* __restrict__ rstd_out,
                                          int H, float eps) {
  __shared__ float red[LN_BLOCK / 64];
  const int row = blockIdx.x;
  short* yr = y + (int64_t)row * H;
  layer_norm_rows<1, true>(
      a, b, w, bias, h, mean_out, rstd_out, red, row, H, eps,
      [&](int, int i, bf16x8 o) { *reinterpret_cast<bf16x8*>(yr + i) = o; });
}

// ---------------------------------------------------------------- backward dx
// dx = (wdy - mean(wdy) - xhat * mean(wdy*xhat)) * rstd, plus the residual
// gradient dh when HAS_DH (add_layer_norm_bwd with a dh).  One workgroup per
// row; launched for rows wider than LNF_MAX_H, and the definition of dx that
// the fused kernel below reproduces.
template <bool HAS_DH>
__global__ void layer_norm_bwd_dx_kernel(
    const short* __restrict__ dy, const short* __restrict__ dh,
    const short* __restrict__ x, const short* __restrict__ w,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    short* __restrict__ dx, int H) {
  const int row = blockIdx.x;
  const short* dyr = dy + (int64_t)row * H;
  const short* dhr = HAS_DH ? dh + (int64_t)row * H : nullptr;
  const short* xr = x + (int64_t)row * H;
  short* dxr = dx + (int64_t)row * H;
  const float mean = mean_in[row], rstd = rstd_in[row];
  __shared__ float red[LN_BLOCK / 64];

  // two passes over the row (L2-resident for these row sizes; a
  // register-cached single-read variant measured NEUTRAL-to-worse —
  // the extra VGPRs bought nothing).
  float c1 = 0.f, c2 = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += LN_BLOCK * 8) {
    bf16x8 dv = *reinterpret_cast<const bf16x8*>(dyr + i);
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(xr + i);
    bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float wdy = bf2f(dv[j]) * bf2f(wv[j]);
      float xhat = (bf2f(xv[j]) - mean) * rstd;
      c1 += wdy;
      c2 += wdy * xhat;
    }
  }
  c1 = block_reduce_sum(c1, red) / H;
  c2 = block_reduce_sum(c2, red) / H;

  for (int i = threadIdx.x * 8; i < H; i += LN_BLOCK * 8) {
    bf16x8 dv = *reinterpret_cast<const bf16x8*>(dyr + i);
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(xr + i);
    bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + i);
    bf16x8 hv;
    if (HAS_DH) hv = *reinterpret_cast<const bf16x8*>(dhr + i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float wdy = bf2f(dv[j]) * bf2f(wv[j]);
      float xhat = (bf2f(xv[j]) - mean) * rstd;
      float g = (wdy - c1 - xhat * c2) * rstd;
      if (HAS_DH) g += bf2f(hv[j]);
      o[j] = f2bf(g);
    }
    *reinterpret_cast<bf16x8*>(dxr + i) = o;
  }
}

// ------------------------------------------------- backward, one pass (fused)
// dx, dw and db from one read of dy, h (and dh), for H <= LNF_MAX_H.  Block p
// owns stripe p, a contiguous range of rows; thread t owns columns
// t*8 .. t*8+7 of each 2048-column trip, for every row of the stripe.  A row
// is loaded once into registers, goes through the two block reductions and
// the dx arithmetic of layer_norm_bwd_dx_kernel — same expressions, same
// order of each thread's partial sums, so dx has the same bits — and adds
// dy*xhat and dy into the thread's fp32 column sums, rows in order.  The
// sums leave as [P, H] partials for colsum_finalize_kernel.
//
// Stripe count and rows side by side (LNF_ROWS rows' loads in flight per
// thread), chosen from the sweep at [32768, 2560] recorded in
// docs/BENCHMARK.md.  More stripes put more bytes in flight and cost a larger
// [P, H] partial round trip; 1024 is one block per SIMD slot at the 4
// waves/SIMD that one row at a time leaves the two-trip kernel.  Two rows
// need 164-180 VGPRs, 2-3 waves/SIMD, and measured slower at 1024 stripes.
// The stripe count fixes the summation order of dw and db.
#define LNF_MAX_H 4096  // two trips: 4 waves/SIMD; four would leave 2
#define LNF_STRIPES 1024
#define LNF_ROWS 1

template <int RI, bool HAS_DH, int TRIPS>
__device__ __forceinline__ void layer_norm_bwd_fused_rows(
    const short* __restrict__ dy, const short* __restrict__ dh,
    const short* __restrict__ x, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, short* __restrict__ dx,
    const bf16x8 (&wv)[TRIPS], float (&dw)[TRIPS][8], float (&db)[TRIPS][8],
    float* red, int64_t row, int H) {
  bf16x8 dv[RI][TRIPS], xv[RI][TRIPS], hv[RI][TRIPS];
  float mean[RI], rstd[RI];
#pragma unroll
  for (int u = 0; u < RI; ++u) {
    mean[u] = mean_in[row + u];
    rstd[u] = rstd_in[row + u];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int i = (t * LN_BLOCK + threadIdx.x) * 8;
      if (i < H) {
        const int64_t at = (row + u) * H + i;
        dv[u][t] = *reinterpret_cast<const bf16x8*>(dy + at);
        xv[u][t] = *reinterpret_cast<const bf16x8*>(x + at);
        if (HAS_DH) hv[u][t] = *reinterpret_cast<const bf16x8*>(dh + at);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RI; ++u) {
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      if ((t * LN_BLOCK + threadIdx.x) * 8 < H) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float wdy = bf2f(dv[u][t][j]) * bf2f(wv[t][j]);
          float xhat = (bf2f(xv[u][t][j]) - mean[u]) * rstd[u];
          c1 += wdy;
          c2 += wdy * xhat;
        }
      }
    }
    c1 = block_reduce_sum(c1, red) / H;
    c2 = block_reduce_sum(c2, red) / H;
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int i = (t * LN_BLOCK + threadIdx.x) * 8;
      if (i < H) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float d = bf2f(dv[u][t][j]);
          float wdy = d * bf2f(wv[t][j]);
          float xhat = (bf2f(xv[u][t][j]) - mean[u]) * rstd[u];
          float g = (wdy - c1 - xhat * c2) * rstd[u];
          if (HAS_DH) g += bf2f(hv[u][t][j]);
          o[j] = f2bf(g);
          dw[t][j] += d * xhat;
          db[t][j] += d;
        }
        *reinterpret_cast<bf16x8*>(dx + (row + u) * H + i) = o;
      }
    }
  }
}

template <bool HAS_DH, int TRIPS>
__global__ void __launch_bounds__(LN_BLOCK)
layer_norm_bwd_fused_kernel(const short* __restrict__ dy,
                            const short* __restrict__ dh,
                            const short* __restrict__ x,
                            const short* __restrict__ w,
                            const float* __restrict__ mean_in,
                            const float* __restrict__ rstd_in,
                            short* __restrict__ dx,
                            float* __restrict__ dw_part,
                            float* __restrict__ db_part, int64_t N, int H) {
  __shared__ float red[LN_BLOCK / 64];
  const int p = blockIdx.x;
  const int P = gridDim.x;
  const int64_t r0 = (int64_t)p * N / P, r1 = (int64_t)(p + 1) * N / P;
  bf16x8 wv[TRIPS];
  float dw[TRIPS][8], db[TRIPS][8];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int i = (t * LN_BLOCK + threadIdx.x) * 8;
    if (i < H) wv[t] = *reinterpret_cast<const bf16x8*>(w + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[t][j] = db[t][j] = 0.f;
  }
  int64_t row = r0;
  for (; row + LNF_ROWS <= r1; row += LNF_ROWS)
    layer_norm_bwd_fused_rows<LNF_ROWS, HAS_DH, TRIPS>(
        dy, dh, x, mean_in, rstd_in, dx, wv, dw, db, red, row, H);
  for (; row < r1; ++row)
    layer_norm_bwd_fused_rows<1, HAS_DH, TRIPS>(
        dy, dh, x, mean_in, rstd_in, dx, wv, dw, db, red, row, H);
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int i = (t * LN_BLOCK + threadIdx.x) * 8;
    if (i < H) {
      float* dwp = dw_part + (int64_t)p * H + i;
      float* dbp = db_part + (int64_t)p * H + i;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dwp[j] = dw[t][j];
        dbp[j] = db[t][j];
      }
    }
  }
}

// --------------------------------------------- backward dw/db, rows > 4096
// Striped partials: grid (ceil(H / 1024), P); block (c, p) sums stripe p, a
// contiguous range of rows, over its 1024 columns.  Output partial [P, H]
// fp32 for colsum_finalize_kernel.  With layer_norm_bwd_dx_kernel this is
// the backward of rows wider than LNF_MAX_H.
#define LNB_COLS 256  // threads per block, 4 columns each

__global__ void layer_norm_bwd_dwdb_partial(const short* __restrict__ dy,
                                            const short* __restrict__ x,
                                            const float* __restrict__ mean_in,
                                            const float* __restrict__ rstd_in,
                                            float* __restrict__ dw_part,
                                            float* __restrict__ db_part,
                                            int N, int H) {
  // 4 columns per thread (bf16x4 loads — the 1-col scalar version was
  // issue-bound well off the HBM roofline, cf. the dbias partial)
  const int col4 = (blockIdx.x * LNB_COLS + threadIdx.x) * 4;
  const int p = blockIdx.y;  // stripe index
  const int P = gridDim.y;
  // contiguous row range per stripe (DRAM page locality)
  const int64_t r0 = (int64_t)p * N / P, r1 = (int64_t)(p + 1) * N / P;
  if (col4 + 4 <= H) {
    float dw[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t row = r0; row < r1; ++row) {
      float mean = mean_in[row], rstd = rstd_in[row];
      bf16x4 dv = *reinterpret_cast<const bf16x4*>(dy + row * H + col4);
      bf16x4 xv = *reinterpret_cast<const bf16x4*>(x + row * H + col4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = bf2f(dv[j]);
        dw[j] += d * (bf2f(xv[j]) - mean) * rstd;
        db[j] += d;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dw_part[(int64_t)p * H + col4 + j] = dw[j];
      db_part[(int64_t)p * H + col4 + j] = db[j];
    }
  } else if (col4 < H) {
    for (int c = col4; c < H; ++c) {
      float dw = 0.f, db = 0.f;
      for (int64_t row = r0; row < r1; ++row) {
        float mean = mean_in[row], rstd = rstd_in[row];
        float d = bf2f(dy[row * H + c]);
        dw += d * (bf2f(x[row * H + c]) - mean) * rstd;
        db += d;
      }
      dw_part[(int64_t)p * H + c] = dw;
      db_part[(int64_t)p * H + c] = db;
    }
  }
}

// ---------------------------------------------------------------- launchers
extern "C" {

hipError_t launch_layer_norm_fwd(const void* x, const void* w, const void* b,
                                 void* y, float* mean, float* rstd, int64_t N,
                                 int64_t H, float eps, hipStream_t stream) {
  layer_norm_fwd_kernel<<<dim3((uint32_t)N), dim3(LN_BLOCK), 0, stream>>>(
      (const short*)x, (const short*)w, (const short*)b, (short*)y, mean,
      rstd, (int)H, eps);
  return hipGetLastError();
}

int layer_norm_bwd_stripes(int64_t N, int64_t H) {
  if (H <= LNF_MAX_H) return (int)min((int64_t)LNF_STRIPES, N);
  // the dw/db partial kernel: enough (stripes x 256-column chunks) blocks to
  // fill 256 CUs
  const int64_t p = max((int64_t)64, 2048 / (H / 256));
  return (int)min(min(p, N), (int64_t)512);
}

hipError_t launch_layer_norm_bwd(const void* dy, const void* dh,
                                 const void* x, const void* w,
                                 const float* mean, const float* rstd,
                                 void* dx, float* dw_part, float* db_part,
                                 int64_t N, int64_t H, hipStream_t stream) {
  const int P = layer_norm_bwd_stripes(N, H);
  if (H <= LNF_MAX_H) {
    const bool one_trip = H <= LN_BLOCK * 8;
    auto kernel =
        dh != nullptr
            ? (one_trip ? layer_norm_bwd_fused_kernel<true, 1>
                        : layer_norm_bwd_fused_kernel<true, 2>)
            : (one_trip ? layer_norm_bwd_fused_kernel<false, 1>
                        : layer_norm_bwd_fused_kernel<false, 2>);
    kernel<<<dim3(P), dim3(LN_BLOCK), 0, stream>>>(
        (const short*)dy, (const short*)dh, (const short*)x, (const short*)w,
        mean, rstd, (short*)dx, dw_part, db_part, N, (int)H);
    return hipGetLastError();
  }
  auto dx_kernel = dh != nullptr ? layer_norm_bwd_dx_kernel<true>
                                 : layer_norm_bwd_dx_kernel<false>;
  dx_kernel<<<dim3((uint32_t)N), dim3(LN_BLOCK), 0, stream>>>(
      (const short*)dy, (const short*)dh, (const short*)x, (const short*)w,
      mean, rstd, (short*)dx, (int)H);
  dim3 grid((uint32_t)ceil_div(H, LNB_COLS * 4), P);
  layer_norm_bwd_dwdb_partial<<<grid, dim3(LNB_COLS), 0, stream>>>(
      (const short*)dy, (const short*)x, mean, rstd, dw_part, db_part,
      (int)N, (int)H);
  return hipGetLastError();
}

hipError_t launch_add_layer_norm_fwd(const void* a, const void* b,
                                     const void* w, const void* bias,
                                     void* h, void* y, float* mean,
                                     float* rstd, int64_t N, int64_t H,
                                     float eps, hipStream_t stream) {
  add_layer_norm_fwd_kernel<<<dim3((uint32_t)N), dim3(LN_BLOCK), 0,
                              stream>>>(
      (const short*)a, (const short*)b, (const short*)w, (const short*)bias,
      (short*)h, (short*)y, mean, rstd, (int)H, eps);
  return hipGetLastError();
}

}  // extern "C"
