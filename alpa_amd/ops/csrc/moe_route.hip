// Top-2 MoE routing, dispatch and combine for bf16 activations (gfx950).
//
// Everything here has shapes fixed by (N, E, C, H) and reads nothing back
// to the host, so a step that holds a MoE layer never blocks on the device.
// It is deterministic: the only cross-thread sums are integer counts and
// fixed-order fp32 partials, and every output element has one writer.
//
// Routing runs as three launches over 256-token blocks:
//   top2   per token: idx1/idx2 (lowest index wins ties), w1/w2, and the
//          token's stable rank among the block's tokens that chose the
//          same expert; per block: the expert histograms of both choices
//          and the column sums of softmax(logits) for the aux loss
//   scan   one block: exclusive scan of the block histograms per expert,
//          count1, aux
//   slots  per token: position = scanned offset + in-block rank (second
//          choices start behind min(count1, C)), slot or -1, src[slot] = t
// Dispatch and combine are one gather pass each with 16-byte accesses.
#include "common.h"
#include "launchers.h"

#define MOE_BLOCK 256
#define MOE_WAVES (MOE_BLOCK / 64)
#define MOE_MAX_E 128

// Stable rank of this lane among the wave's active lanes with the same
// expert; the wave's count per expert goes to cnt[e] (pre-zeroed LDS).
// One ballot round per distinct expert in the wave.  The loop condition is
// a ballot, so it is wave-uniform.
__device__ __forceinline__ int wave_rank(int e, bool active, int* cnt) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int rank = 0;
  bool todo = active;
  for (;;) {
    const unsigned long long rem = __ballot(todo);
    if (rem == 0ull) break;
    const int leader = __ffsll(rem) - 1;
    const int e0 = __shfl(e, leader, 64);
    const bool mine = todo && e == e0;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      rank = __popcll(m & below);
      if (lane == leader) cnt[e0] = __popcll(m);
      todo = false;
    }
  }
  return rank;
}

// ------------------------------------------------------------------ top-2
// logits [N, E] bf16.  One token per thread.  rank1/rank2 are written into
// the slot1/slot2 buffers and turned into slots by moe_slots_kernel.
// hist1/hist2 [nblocks, E] int32, ppart [nblocks, E] fp32.
__global__ __launch_bounds__(MOE_BLOCK) void moe_top2_kernel(
    const short* __restrict__ logits, float* __restrict__ w1,
    float* __restrict__ w2, int* __restrict__ idx1, int* __restrict__ idx2,
    int* __restrict__ rank1, int* __restrict__ rank2, int* __restrict__ hist1,
    int* __restrict__ hist2, float* __restrict__ ppart, int N, int E,
    int Epad) {
  __shared__ float s_m[MOE_BLOCK];
  __shared__ float s_inv[MOE_BLOCK];
  __shared__ float s_part[MOE_BLOCK];
  __shared__ int s_cnt[2][MOE_WAVES][MOE_MAX_E];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * MOE_BLOCK;
  const int64_t t = t0 + tid;
  const bool active = t < N;

  for (int i = tid; i < 2 * MOE_WAVES * MOE_MAX_E; i += MOE_BLOCK)
    (&s_cnt[0][0][0])[i] = 0;
  __syncthreads();

  // Running top-2 with strict '>' only: the lowest index wins a tie, and
  // a NaN never wins a comparison, so i1 != i2 and both stay in [0, E)
  // whatever the row holds.
  int i1 = 0, i2 = 1;
  float m = 0.f, inv = 0.f;
  if (active) {
    const short* row = logits + t * E;
    float b1 = bf2f(row[0]);
    float b2 = bf2f(row[1]);
    if (b2 > b1) {
      float tb = b1;
      b1 = b2;
      b2 = tb;
      i1 = 1;
      i2 = 0;
    }
    for (int e = 2; e < E; ++e) {
      const float v = bf2f(row[e]);
      if (v > b1) {
        b2 = b1;
        i2 = i1;
        b1 = v;
        i1 = e;
      } else if (v > b2) {
        b2 = v;
        i2 = e;
      }
    }
    m = b1;
    float sum = 0.f;
    for (int e = 0; e < E; ++e) sum += __expf(bf2f(row[e]) - m);
    inv = 1.0f / sum;
    const float p1 = __expf(b1 - m) * inv;
    const float p2 = __expf(b2 - m) * inv;
    const float den = p1 + p2;
    w1[t] = p1 / den;
    w2[t] = p2 / den;
    idx1[t] = i1;
    idx2[t] = i2;
  }
  s_m[tid] = m;
  s_inv[tid] = inv;

  int r1 = wave_rank(i1, active, s_cnt[0][wave]);
  int r2 = wave_rank(i2, active, s_cnt[1][wave]);
  __syncthreads();
  for (int w = 0; w < wave; ++w) {
    r1 += s_cnt[0][w][i1];
    r2 += s_cnt[1][w][i2];
  }
  if (active) {
    rank1[t] = r1;
    rank2[t] = r2;
  }
  if (tid < E) {
    int c1 = 0, c2 = 0;
#pragma unroll
    for (int w = 0; w < MOE_WAVES; ++w) {
      c1 += s_cnt[0][w][tid];
      c2 += s_cnt[1][w][tid];
    }
    hist1[(int64_t)blockIdx.x * E + tid] = c1;
    hist2[(int64_t)blockIdx.x * E + tid] = c2;
  }

  // Column sums of p over the block's rows, in a fixed order: thread
  // (g, e) adds rows g, g+G, ...; then thread e adds the G partials.
  // Lanes of one row group read consecutive columns.
  const int e = tid & (Epad - 1);
  const int g = tid / Epad;
  const int G = MOE_BLOCK / Epad;
  float acc = 0.f;
  if (e < E) {
    for (int r = g; r < MOE_BLOCK && t0 + r < N; r += G)
      acc += __expf(bf2f(logits[(t0 + r) * E + e]) - s_m[r]) * s_inv[r];
  }
  s_part[tid] = acc;
  __syncthreads();
  if (tid < E) {
    float s = 0.f;
    for (int gg = 0; gg < G; ++gg) s += s_part[gg * Epad + tid];
    ppart[(int64_t)blockIdx.x * E + tid] = s;
  }
}

// ------------------------------------------------------------------- scan
// One block.  Thread e turns column e of hist1/hist2 into exclusive
// prefixes in place, writes count1[e], and thread 0 adds up aux in index
// order.  psum [E] is the column sum of p over all tokens.
__global__ __launch_bounds__(MOE_MAX_E) void moe_scan_kernel(
    int* __restrict__ hist1, int* __restrict__ hist2,
    const float* __restrict__ psum, int* __restrict__ count1,
    float* __restrict__ aux, int nblocks, int N, int E) {
  __shared__ float s_term[MOE_MAX_E];
  const int e = threadIdx.x;
  if (e < E) {
    int run1 = 0, run2 = 0;
    for (int b = 0; b < nblocks; ++b) {
      const int64_t i = (int64_t)b * E + e;
      const int c1 = hist1[i], c2 = hist2[i];
      hist1[i] = run1;
      hist2[i] = run2;
      run1 += c1;
      run2 += c2;
    }
    count1[e] = run1;
    s_term[e] = (psum[e] / (float)N) * ((float)run1 / (float)N);
  }
  __syncthreads();
  if (e == 0) {
    float s = 0.f;
    for (int i = 0; i < E; ++i) s += s_term[i];
    *aux = (float)E * s;
  }
}

// ------------------------------------------------------------------ slots
// slot1/slot2 hold the in-block ranks on entry.  src is pre-filled with -1;
// each kept (token, choice) owns one slot, so src has one writer per entry.
__global__ __launch_bounds__(MOE_BLOCK) void moe_slots_kernel(
    const int* __restrict__ idx1, const int* __restrict__ idx2,
    const int* __restrict__ off1, const int* __restrict__ off2,
    const int* __restrict__ count1, int* __restrict__ slot1,
    int* __restrict__ slot2, int* __restrict__ src, int N, int E,
    int64_t C) {
  const int64_t t = (int64_t)blockIdx.x * MOE_BLOCK + threadIdx.x;
  if (t >= N) return;
  const int e1 = idx1[t], e2 = idx2[t];  // written in range by the top-2
  const int64_t pos1 = (int64_t)off1[(int64_t)blockIdx.x * E + e1] + slot1[t];
  const int64_t c1 = count1[e2];
  const int64_t pos2 = (c1 < C ? c1 : C) +
                       off2[(int64_t)blockIdx.x * E + e2] + slot2[t];
  const int s1 = pos1 < C ? (int)(e1 * C + pos1) : -1;
  const int s2 = pos2 < C ? (int)(e2 * C + pos2) : -1;
  slot1[t] = s1;
  slot2[t] = s2;
  if (s1 >= 0) src[s1] = (int)t;
  if (s2 >= 0) src[s2] = (int)t;
}

// --------------------------------------------------------- route backward
// dlogits = p * (dp - sum(dp * p)) + onehot(idx1) * dl1 - onehot(idx2) * dl1
// with dp[e] = daux * E * count1[e] / N^2 and dl1 = (dw1 - dw2) * w1 * w2.
// One token per thread; the softmax is recomputed.
__global__ __launch_bounds__(MOE_BLOCK) void moe_route_bwd_kernel(
    const short* __restrict__ logits, const int* __restrict__ idx1,
    const int* __restrict__ idx2, const float* __restrict__ w1,
    const float* __restrict__ w2, const int* __restrict__ count1,
    const float* __restrict__ dw1, const float* __restrict__ dw2,
    const float* __restrict__ daux, short* __restrict__ dlogits, int N,
    int E) {
  __shared__ float s_dp[MOE_MAX_E];
  if (threadIdx.x < E) {
    s_dp[threadIdx.x] = daux[0] * ((float)E * (float)count1[threadIdx.x] /
                                   ((float)N * (float)N));
  }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * MOE_BLOCK + threadIdx.x;
  if (t >= N) return;
  const short* row = logits + t * E;
  short* out = dlogits + t * E;
  float m = bf2f(row[0]);
  for (int e = 1; e < E; ++e) m = fmaxf(m, bf2f(row[e]));
  float sum = 0.f, dot = 0.f;
  for (int e = 0; e < E; ++e) {
    const float ex = __expf(bf2f(row[e]) - m);
    sum += ex;
    dot += ex * s_dp[e];
  }
  const float inv = 1.0f / sum;
  dot *= inv;
  const int i1 = idx1[t], i2 = idx2[t];
  const float a = w1[t], b = w2[t];
  const float dl1 = (dw1[t] - dw2[t]) * a * b;
  for (int e = 0; e < E; ++e) {
    const float p = __expf(bf2f(row[e]) - m) * inv;
    float g = p * (s_dp[e] - dot);
    if (e == i1) g += dl1;
    if (e == i2) g -= dl1;
    out[e] = f2bf(g);
  }
}

// --------------------------------------------------------------- dispatch
// out[s] = x[src[s]] (zeros for an empty or out-of-range src), one bf16x8
// per thread per trip.  With slot1/w1/w2 given, row s is scaled by the gate
// weight of the choice that put its token there: the combine's dy.
__global__ __launch_bounds__(MOE_BLOCK) void moe_dispatch_kernel(
    const short* __restrict__ x, const int* __restrict__ src,
    const int* __restrict__ slot1, const float* __restrict__ w1,
    const float* __restrict__ w2, short* __restrict__ out, int64_t S,
    int64_t N, int H8) {
  const int64_t total = S * H8;
  const int64_t stride = (int64_t)gridDim.x * MOE_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * MOE_BLOCK + threadIdx.x; i < total;
       i += stride) {
    const int64_t s = i / H8;
    const int c = (int)(i - s * H8);
    const int t = src[s];
    bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t >= 0 && t < N) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(x + ((int64_t)t * H8 + c) * 8);
      if (slot1 != nullptr) {
        const float w = (slot1[t] == s) ? w1[t] : w2[t];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(w * bf2f(v[j]));
      } else {
        o = v;
      }
    }
    *reinterpret_cast<bf16x8*>(out + i * 8) = o;
  }
}

// ---------------------------------------------------------------- combine
// out[t] = w1[t] * y[slot1[t]] + w2[t] * y[slot2[t]], dropped terms
// skipped, fp32 sum rounded once.  w1 == nullptr means unit weights: the
// dispatch's dx.
__global__ __launch_bounds__(MOE_BLOCK) void moe_combine_kernel(
    const short* __restrict__ y, const float* __restrict__ w1,
    const float* __restrict__ w2, const int* __restrict__ slot1,
    const int* __restrict__ slot2, short* __restrict__ out, int64_t N,
    int64_t S, int H8) {
  const int64_t total = N * H8;
  const int64_t stride = (int64_t)gridDim.x * MOE_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * MOE_BLOCK + threadIdx.x; i < total;
       i += stride) {
    const int64_t t = i / H8;
    const int c = (int)(i - t * H8);
    const int s1 = slot1[t], s2 = slot2[t];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (s1 >= 0 && s1 < S) {
      const float a = (w1 != nullptr) ? w1[t] : 1.0f;
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(y + ((int64_t)s1 * H8 + c) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = a * bf2f(v[j]);
    }
    if (s2 >= 0 && s2 < S) {
      const float b = (w2 != nullptr) ? w2[t] : 1.0f;
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(y + ((int64_t)s2 * H8 + c) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += b * bf2f(v[j]);
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
    *reinterpret_cast<bf16x8*>(out + i * 8) = o;
  }
}

// ------------------------------------------------- combine weight gradient
// dw_k[t] = <dout[t], y[slot_k[t]]> in fp32, 0 when dropped.  One wave per
// token, both dots in one pass over dout[t].
__global__ __launch_bounds__(MOE_BLOCK) void moe_combine_dw_kernel(
    const short* __restrict__ dout, const short* __restrict__ y,
    const int* __restrict__ slot1, const int* __restrict__ slot2,
    float* __restrict__ dw1, float* __restrict__ dw2, int64_t N, int64_t S,
    int H8) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * MOE_WAVES + (threadIdx.x >> 6);
  if (t >= N) return;  // wave-uniform
  const int s1 = slot1[t], s2 = slot2[t];
  const bool k1 = s1 >= 0 && s1 < S, k2 = s2 >= 0 && s2 < S;
  float d1 = 0.f, d2 = 0.f;
  for (int c = lane; c < H8; c += 64) {
    const bf16x8 g =
        *reinterpret_cast<const bf16x8*>(dout + (t * H8 + c) * 8);
    if (k1) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(y + ((int64_t)s1 * H8 + c) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) d1 += bf2f(g[j]) * bf2f(v[j]);
    }
    if (k2) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(y + ((int64_t)s2 * H8 + c) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) d2 += bf2f(g[j]) * bf2f(v[j]);
    }
  }
  d1 = wave_reduce_sum(d1);
  d2 = wave_reduce_sum(d2);
  if (lane == 0) {
    dw1[t] = d1;
    dw2[t] = d2;
  }
}

// ---------------------------------------------------------------- launchers
// Callers guarantee N >= 1, 2 <= E <= 128, E*C < 2^31, H % 8 == 0, so no
// grid here is empty.
static inline uint32_t moe_flat_grid(int64_t total) {
  // memory-bound gathers: cap the grid and stride the rest
  int64_t blocks = ceil_div(total, MOE_BLOCK);
  return (uint32_t)(blocks < 4096 ? blocks : 4096);
}

extern "C" {

hipError_t launch_moe_route(const void* logits, float* w1, float* w2,
                            int* idx1, int* idx2, int* slot1, int* slot2,
                            int* hist1, int* hist2, float* ppart, int64_t N,
                            int64_t E, hipStream_t stream) {
  int Epad = 2;
  while (Epad < E) Epad *= 2;
  const uint32_t nblocks = (uint32_t)ceil_div(N, MOE_BLOCK);
  moe_top2_kernel<<<dim3(nblocks), dim3(MOE_BLOCK), 0, stream>>>(
      (const short*)logits, w1, w2, idx1, idx2, slot1, slot2, hist1, hist2,
      ppart, (int)N, (int)E, Epad);
  return hipGetLastError();
}

hipError_t launch_moe_slots(const int* idx1, const int* idx2, int* hist1,
                            int* hist2, const float* psum, int* count1,
                            float* aux, int* slot1, int* slot2, int* src,
                            int64_t N, int64_t E, int64_t C,
                            hipStream_t stream) {
  const uint32_t nblocks = (uint32_t)ceil_div(N, MOE_BLOCK);
  // empty slots read -1: all-ones bytes, set on the stream ahead of the
  // kernels so that a captured graph replays it every call
  hipError_t err = hipMemsetAsync(src, 0xFF, (size_t)(E * C) * sizeof(int),
                                  stream);
  if (err != hipSuccess) return err;
  moe_scan_kernel<<<dim3(1), dim3(MOE_MAX_E), 0, stream>>>(
      hist1, hist2, psum, count1, aux, (int)nblocks, (int)N, (int)E);
  moe_slots_kernel<<<dim3(nblocks), dim3(MOE_BLOCK), 0, stream>>>(
      idx1, idx2, hist1, hist2, count1, slot1, slot2, src, (int)N, (int)E, C);
  return hipGetLastError();
}

hipError_t launch_moe_route_bwd(const void* logits, const int* idx1,
                                const int* idx2, const float* w1,
                                const float* w2, const int* count1,
                                const float* dw1, const float* dw2,
                                const float* daux, void* dlogits, int64_t N,
                                int64_t E, hipStream_t stream) {
  const uint32_t nblocks = (uint32_t)ceil_div(N, MOE_BLOCK);
  moe_route_bwd_kernel<<<dim3(nblocks), dim3(MOE_BLOCK), 0, stream>>>(
      (const short*)logits, idx1, idx2, w1, w2, count1, dw1, dw2, daux,
      (short*)dlogits, (int)N, (int)E);
  return hipGetLastError();
}

hipError_t launch_moe_dispatch(const void* x, const int* src,
                               const int* slot1_or_null,
                               const float* w1_or_null,
                               const float* w2_or_null, void* out, int64_t S,
                               int64_t N, int64_t H, hipStream_t stream) {
  moe_dispatch_kernel<<<dim3(moe_flat_grid(S * (H / 8))), dim3(MOE_BLOCK), 0,
                        stream>>>((const short*)x, src, slot1_or_null,
                                  w1_or_null, w2_or_null, (short*)out, S, N,
                                  (int)(H / 8));
  return hipGetLastError();
}

hipError_t launch_moe_combine(const void* y, const float* w1_or_null,
                              const float* w2_or_null, const int* slot1,
                              const int* slot2, void* out, int64_t N,
                              int64_t S, int64_t H, hipStream_t stream) {
  moe_combine_kernel<<<dim3(moe_flat_grid(N * (H / 8))), dim3(MOE_BLOCK), 0,
                       stream>>>((const short*)y, w1_or_null, w2_or_null,
                                 slot1, slot2, (short*)out, N, S,
                                 (int)(H / 8));
  return hipGetLastError();
}

hipError_t launch_moe_combine_dw(const void* dout, const void* y,
                                 const int* slot1, const int* slot2,
                                 float* dw1, float* dw2, int64_t N, int64_t S,
                                 int64_t H, hipStream_t stream) {
  const uint32_t nblocks = (uint32_t)ceil_div(N, MOE_WAVES);
  moe_combine_dw_kernel<<<dim3(nblocks), dim3(MOE_BLOCK), 0, stream>>>(
      (const short*)dout, (const short*)y, slot1, slot2, dw1, dw2, N, S,
      (int)(H / 8));
  return hipGetLastError();
}

}  // extern "C"
