// Split-KV decode attention (bf16, one query row per (batch, head)) for
// gfx950: flash-decoding in two launches, no MFMA, no LDS staging of K or V.
//
// The prefill kernel (attention.hip) gives one workgroup 128 query rows of
// one (batch, head); with a single query row its grid is 1 x B*H and each
// workgroup walks its head's whole cache serially.  Here the KV axis is cut
// into fixed chunks of CHUNK keys:
//
//   partial  grid (n_chunks, B*H), 256 threads.  The workgroup of chunk c
//            handles keys [c*CHUNK, min((c+1)*CHUNK, len_b)): scores, the
//            chunk max m_c, l_c = sum exp(s - m_c) and the unnormalised
//            acc_c[D] = sum exp(s - m_c) v, written to an fp32 workspace.
//            A chunk that starts at or past len_b returns before any load
//            or store.
//   combine  grid B*H.  Merges chunks 0 .. ceil(len_b/CHUNK)-1 in ascending
//            order: M = max m_c, w_c = exp(m_c - M),
//            o = sum w_c acc_c / sum w_c l_c, lse = M + log sum w_c l_c.
//            It never reads the workspace of a dead chunk.  No atomics, no
//            in-launch hand-off (as skinny_gemm's finalize).
//
// With n_chunks == 1 the partial kernel finishes the row itself through the
// same attn_decode_finish(): one chunk merges with w = 1 exactly, so the
// bits equal those of the two-launch path.
//
// Loads: a key row of D bf16 is read by Dp/8 adjacent lanes, 16 bytes each,
// so one wave instruction covers 64/(Dp/8) whole rows contiguously and the
// four waves of a round cover 4x that; up to 8 rows per lane are in flight
// before the first wait.  Rows at or past len_b and columns at or past D are
// never loaded.  Everything after the loads is fp32: the dot products are
// plain FMAs, P is not rounded, o is rounded to bf16 once.  LDS holds only
// the chunk's scores/probabilities and the cross-wave reductions.
//
// Bit invariance: which lane adds what in which order is a function of the
// position inside the chunk and of len_b alone, and CHUNK depends on the
// head-dim instantiation only.  So o[b, h] and lse[b, h] depend on that
// slot's q, its first len_b rows of k and v, len_b, D, scale and the slope,
// and not on B, H, Skv, what lies past len_b, or the other slots.
//
// CHUNK = 128 for every instantiation, by a sweep of {128, 256, 512} on one
// MI355X over H 40/56 at D 128 and H 24 at D 256, batch 1/8/32, Skv
// 128/512/2048, partial + combine timed together.  128 wins wherever the
// grid is small (batch 1, Skv 512: 9.7 vs 16.0 vs 14.0 us at D 128, 13.3 vs
// 17.8 vs 25.4 us at D 256: a workgroup's time is its chain of load batches,
// and a 128-key chunk has one per operand) and stays within 5 % of the best
// at batch 32, Skv 2048 (236 vs 232 vs 227 us; 282 vs 272 vs 268 us at
// D 256); its worst case is 15 % behind 512 (H 56, batch 8, Skv 512).
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage), partial
// kernel at Dp 64 / 128 / 256: 41 / 62 / 66-71 VGPRs, 8 / 8 / 7 waves per
// SIMD (the intent: several workgroups per CU, so that a CU has loads of
// more than one chunk in flight), 1552 / 2576 / 4624 B of LDS, no scratch.
// Combine kernel: 10 VGPRs, 8 waves per SIMD, no LDS, no scratch.
#include "attn_strides.h"
#include "common.h"
#include "launchers.h"

#define DEC_THREADS 256
#define DEC_WAVES (DEC_THREADS / 64)

// Keys per chunk for the instantiation padded to Dp.  A compile-time
// constant per Dp: it must never depend on B, H, Skv or the device, or the
// invariance above is gone.  ops.DECODE_ATTN_CHUNK mirrors it.
template <int Dp>
struct DecodeChunk {
  static constexpr int value = 128;
};

__device__ __forceinline__ void unpack_bf16x8(bf16x8 x, float* f) {
  union {
    bf16x8 v;
    uint32_t u[4];
  } c;
  c.v = x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(c.u[i] << 16);
    f[2 * i + 1] = __uint_as_float(c.u[i] & 0xffff0000u);
  }
}

// The one place a row is normalised, shared by the combine kernel and the
// single-chunk shortcut.  Contraction is off so that both callers round in
// the same places whatever surrounds the call.
__device__ __forceinline__ void attn_decode_finish(float a, float L, float M,
                                                   short* o_elem,
                                                   float* lse_elem) {
#pragma clang fp contract(off)
  const float inv_l = (L > 0.f) ? 1.0f / L : 0.f;
  if (o_elem != nullptr) *o_elem = f2bf(a * inv_l);
  if (lse_elem != nullptr) {
    const float lg = __logf(L);
    *lse_elem = (L > 0.f) ? M + lg : -INFINITY;
  }
}

__device__ __forceinline__ int decode_len(const int* kv_lens, int batch,
                                          int Skv) {
  const int len = kv_lens != nullptr ? kv_lens[batch] : Skv;
  return min(max(len, 0), Skv);
}

// Dp: head dim padded to 64/128/256; CH: keys per chunk; AL: ALiBi bias.
// ws: fp32 [B*H, n_chunks, 2] of (m_c, l_c), then [B*H, n_chunks, D] of
// acc_c; unused when gridDim.x == 1.
template <int Dp, int CH, bool AL>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_partial_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, float* __restrict__ ws, int H, int Skv,
    int D, float scale, const float* __restrict__ alibi,
    const int* __restrict__ kv_lens, AttnStrides st) {
  constexpr int LPR = Dp / 8;            // lanes per key row
  constexpr int RPI = 64 / LPR;          // rows per wave load instruction
  constexpr int RPR = DEC_WAVES * RPI;   // rows per workgroup round
  constexpr int ROUNDS = CH / RPR;
  constexpr int U = ROUNDS < 8 ? ROUNDS : 8;  // rounds in flight
  static_assert(Dp <= DEC_THREADS && CH % RPR == 0 && ROUNDS % U == 0,
                "chunk must be whole rounds");

  const int c = blockIdx.x, n_chunks = gridDim.x;
  const int bh = blockIdx.y;
  const int batch = bh / H, head = bh % H;
  const bool direct = n_chunks == 1;
  const int len = decode_len(kv_lens, batch, Skv);
  const int start = c * CH;
  short* op = o + batch * st.ob + head * st.oh;

  if (start >= len) {
    // a dead chunk: nothing is loaded and nothing written, unless this
    // workgroup is the whole launch and the slot is empty
    if (direct) {
      if ((int)threadIdx.x < D) op[threadIdx.x] = 0;
      if (threadIdx.x == 0) lse_out[bh] = -INFINITY;
    }
    return;
  }
  const int n = min(CH, len - start);  // live rows of this chunk

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane / LPR;          // which of the instruction's rows
  const int dg = (lane % LPR) * 8;     // this lane's 8 head-dim columns
  const bool col_ok = dg < D;          // D % 8 == 0: then dg + 8 <= D

  __shared__ float s_lds[CH];          // scores, then probabilities
  __shared__ float red[DEC_WAVES][Dp];
  __shared__ float rbuf[DEC_WAVES];

  float qf[8];
  {
    bf16x8 qr = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok)
      qr = *reinterpret_cast<const bf16x8*>(q + batch * st.qb +
                                            head * st.qh + dg);
    unpack_bf16x8(qr, qf);
  }
  const short* kp = k + batch * st.kb + head * st.kh +
                    (int64_t)start * st.ks + dg;
  const short* vp = v + batch * st.vb + head * st.vh +
                    (int64_t)start * st.vs + dg;
  const float al_slope = AL ? alibi[head] : 0.f;

  // ---- scores: row = round * RPR + wave * RPI + grp ----
  float wmax = -INFINITY;
  for (int r0 = 0; r0 < ROUNDS; r0 += U) {
    if (r0 * RPR >= n) break;  // every later row is dead
    bf16x8 kr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = (r0 + u) * RPR + wave * RPI + grp;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kr[u] = z;
      if (row < n && col_ok)
        kr[u] = *reinterpret_cast<const bf16x8*>(kp + (int64_t)row * st.ks);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = (r0 + u) * RPR + wave * RPI + grp;
      float kf[8];
      unpack_bf16x8(kr[u], kf);
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dot = fmaf(kf[j], qf[j], dot);
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) dot += __shfl_xor(dot, off, 64);
      float s = dot * scale;
      if (AL)
        s = fmaf(al_slope, (float)(start + row - (len - 1)), s);
      s = (row < n) ? s : -INFINITY;
      if (dg == 0) s_lds[row] = s;
      wmax = fmaxf(wmax, s);
    }
  }
  const float m = block_reduce_max(wmax, rbuf);  // also publishes s_lds

  // ---- probabilities in place, fp32 ----
  float lpart = 0.f;
#pragma unroll
  for (int t = threadIdx.x; t < CH; t += DEC_THREADS) {
    float p = 0.f;
    if (t < n) {
      const float s = s_lds[t];
      p = (s == -INFINITY) ? 0.f : __expf(s - m);
    }
    s_lds[t] = p;
    lpart += p;
  }
  const float l = block_reduce_sum(lpart, rbuf);  // also publishes p

  // ---- acc = sum p v, same row -> lane map ----
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < ROUNDS; r0 += U) {
    if (r0 * RPR >= n) break;
    bf16x8 vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = (r0 + u) * RPR + wave * RPI + grp;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      vr[u] = z;
      if (row < n && col_ok)
        vr[u] = *reinterpret_cast<const bf16x8*>(vp + (int64_t)row * st.vs);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = (r0 + u) * RPR + wave * RPI + grp;
      const float p = s_lds[row];  // 0 for a dead row, whose v is 0 too
      float vf[8];
      unpack_bf16x8(vr[u], vf);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
    }
  }
  // the wave's row groups, then the four waves, in a fixed order
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][dg + j] = acc[j];
  }
  __syncthreads();
  const int t = threadIdx.x;
  float a = 0.f;
  if (t < Dp) {
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) a += red[w][t];
  }
  if (direct) {
    attn_decode_finish(a, l, m, t < D ? op + t : nullptr,
                       t == 0 ? lse_out + bh : nullptr);
    return;
  }
  const int64_t slot = (int64_t)bh * n_chunks + c;
  if (t == 0) {
    ws[slot * 2] = m;
    ws[slot * 2 + 1] = l;
  }
  if (t < D)
    ws[(int64_t)gridDim.y * n_chunks * 2 + slot * D + t] = a;
}

// One workgroup per (batch, head); thread t owns head-dim column t.
template <int CH>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_combine_kernel(
    const float* __restrict__ ws, short* __restrict__ o,
    float* __restrict__ lse_out, int H, int Skv, int D, int n_chunks,
    const int* __restrict__ kv_lens, AttnStrides st) {
  const int bh = blockIdx.x;
  const int batch = bh / H, head = bh % H;
  const int t = threadIdx.x;
  const int len = decode_len(kv_lens, batch, Skv);
  const int live = (len + CH - 1) / CH;  // chunks that wrote their slot
  const float* ml = ws + (int64_t)bh * n_chunks * 2;
  const float* accs = ws + (int64_t)gridDim.x * n_chunks * 2 +
                      (int64_t)bh * n_chunks * D;
  float M = -INFINITY;
  for (int c = 0; c < live; ++c) M = fmaxf(M, ml[2 * c]);
  float L = 0.f, a = 0.f;
  for (int c = 0; c < live; ++c) {
    const float mc = ml[2 * c];
    const float w = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    L = fmaf(w, ml[2 * c + 1], L);
    if (t < D) a = fmaf(w, accs[(int64_t)c * D + t], a);
  }
  short* op = o + batch * st.ob + head * st.oh;
  attn_decode_finish(a, L, M, t < D ? op + t : nullptr,
                     t == 0 ? lse_out + bh : nullptr);
}

extern "C" {

int attn_decode_chunk(int64_t D) {
  if (D <= 64) return DecodeChunk<64>::value;
  if (D <= 128) return DecodeChunk<128>::value;
  return DecodeChunk<256>::value;
}

int64_t attn_decode_workspace_floats(int64_t B, int64_t H, int64_t Skv,
                                     int64_t D) {
  const int64_t n_chunks = ceil_div(Skv, attn_decode_chunk(D));
  return n_chunks <= 1 ? 0 : B * H * n_chunks * (D + 2);
}

hipError_t launch_attn_decode(const void* q, const void* k, const void* v,
                              void* o, float* lse, float* ws, int64_t B,
                              int64_t H, int64_t Skv, int64_t D, float scale,
                              const float* alibi, const int* kv_lens,
                              const int64_t* strides, hipStream_t stream) {
  const AttnStrides st = attn_strides(strides);
  if (D <= 0 || D % 8 != 0 || D > 256 || B * H > 65535)
    return hipErrorInvalidValue;
#define DEC_LAUNCH(DP, ALB)                                                \
  do {                                                                     \
    constexpr int CH = DecodeChunk<DP>::value;                             \
    const int64_t n_chunks = Skv > 0 ? ceil_div(Skv, CH) : 1;              \
    dim3 grid((uint32_t)n_chunks, (uint32_t)(B * H));                      \
    attn_decode_partial_kernel<DP, CH, ALB>                                \
        <<<grid, dim3(DEC_THREADS), 0, stream>>>(                          \
            (const short*)q, (const short*)k, (const short*)v, (short*)o,  \
            lse, ws, (int)H, (int)Skv, (int)D, scale, alibi, kv_lens, st); \
    if (n_chunks > 1)                                                      \
      attn_decode_combine_kernel<CH>                                       \
          <<<dim3((uint32_t)(B * H)), dim3(DEC_THREADS), 0, stream>>>(     \
              ws, (short*)o, lse, (int)H, (int)Skv, (int)D, (int)n_chunks, \
              kv_lens, st);                                                \
  } while (0)
#define DEC_DISPATCH(DP)                                                   \
  do {                                                                     \
    if (alibi) DEC_LAUNCH(DP, true);                                       \
    else DEC_LAUNCH(DP, false);                                            \
  } while (0)
  if (D <= 64) {
    DEC_DISPATCH(64);
  } else if (D <= 128) {
    DEC_DISPATCH(128);
  } else {
    DEC_DISPATCH(256);
  }
#undef DEC_DISPATCH
#undef DEC_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
