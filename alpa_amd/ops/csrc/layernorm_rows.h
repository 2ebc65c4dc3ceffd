// The LayerNorm forward row passes, once: layer_norm_fwd, add_layer_norm_fwd
// and add_layer_norm_fp8 are this routine with different template arguments,
// so the bytes they share (h, mean, rstd, the bf16 rounding of y) agree by
// construction.
#pragma once

#include "common.h"

#define LN_BLOCK 256

// The variance sum is a separate multiply and add and the normalize step a
// fused multiply-add.  Left to the compiler, the contraction depends on how
// a caller gets vectorized (one row or several side by side), and callers
// would round differently; spelled out, every caller rounds the same way.
__device__ __forceinline__ float ln_sq_acc(float s, float d) {
#pragma clang fp contract(off)
  float p = d * d;
  return s + p;
}

// RI consecutive rows, starting at `row`, go through the three passes (sum,
// two-pass variance, normalize) side by side: the loads of all RI rows are
// in flight together, each row keeps its own partial sums and its own block
// reductions, so a row's arithmetic does not depend on RI.
//
// ADD: h = a + b is rounded to bf16, written, and normalized (b may be null:
// h = a is still written).  Otherwise a itself is normalized; b and h are
// not touched.  Either way the statistics are those of the ROUNDED row: that
// is the tensor the normalize pass, the backward and every later layer see.
//
// epilogue(u, col, y) receives row `row + u`, columns col..col+7 of
// y = LN(h) * w + bias, already rounded to bf16 — the only place that rounds.
// LN_BLOCK threads; `red` holds LN_BLOCK / 64 floats.
template <int RI, bool ADD, typename Epilogue>
__device__ __forceinline__ void layer_norm_rows(
    const short* __restrict__ a, const short* __restrict__ b,
    const short* __restrict__ w, const short* __restrict__ bias,
    short* __restrict__ h, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, float* red, int64_t row, int H, float eps,
    Epilogue&& epilogue) {
  const short* ar = a + row * H;
  const short* br = (!ADD || b == nullptr) ? nullptr : b + row * H;
  short* hw = ADD ? h + row * H : nullptr;
  // passes 2 and 3 re-read the row (L2): each thread the h elements it
  // wrote itself, so no fence is needed
  const short* hr = ADD ? hw : ar;
  float s[RI], mean[RI], rstd[RI];
#pragma unroll
  for (int u = 0; u < RI; ++u) s[u] = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += LN_BLOCK * 8) {
    bf16x8 hv[RI], bv[RI];
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      hv[u] = *reinterpret_cast<const bf16x8*>(ar + (int64_t)u * H + i);
      if (br != nullptr)
        bv[u] = *reinterpret_cast<const bf16x8*>(br + (int64_t)u * H + i);
    }
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      if (br != nullptr) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          hv[u][j] = f2bf(bf2f(hv[u][j]) + bf2f(bv[u][j]));
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s[u] += bf2f(hv[u][j]);
      if (ADD) *reinterpret_cast<bf16x8*>(hw + (int64_t)u * H + i) = hv[u];
    }
  }
#pragma unroll
  for (int u = 0; u < RI; ++u) mean[u] = block_reduce_sum(s[u], red) / H;
  // variance as the mean of squared deviations.  The one-pass
  // E[x^2] - mean^2 form cancels catastrophically once |mean| >> std
  // (a near-constant row came out with a negative variance, so NaN).
#pragma unroll
  for (int u = 0; u < RI; ++u) s[u] = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += LN_BLOCK * 8) {
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      bf16x8 hv = *reinterpret_cast<const bf16x8*>(hr + (int64_t)u * H + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[u] = ln_sq_acc(s[u], bf2f(hv[j]) - mean[u]);
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
  for (int i = threadIdx.x * 8; i < H; i += LN_BLOCK * 8) {
    const bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + i);
    const bf16x8 cv = *reinterpret_cast<const bf16x8*>(bias + i);
#pragma unroll
    for (int u = 0; u < RI; ++u) {
      bf16x8 hv = *reinterpret_cast<const bf16x8*>(hr + (int64_t)u * H + i);
      bf16x8 y;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = (bf2f(hv[j]) - mean[u]) * rstd[u];
        y[j] = f2bf(__builtin_fmaf(xhat, bf2f(wv[j]), bf2f(cv[j])));
      }
      epilogue(u, i, y);
    }
  }
}
