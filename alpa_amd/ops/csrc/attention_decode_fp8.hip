// Split-KV decode attention over an e4m3 KV cache with one fp32 scale per
// key row and per value row (the format kv_cache_fp8.hip writes), for gfx950.
//
// The launch structure is that of attention_decode.hip, whose header
// describes it: partial grid (n_chunks, B*H) with 256 threads, CHUNK keys
// per workgroup from DecodeChunk<Dp>, the same fp32 workspace, the same
// combine kernel and the same direct finish when n_chunks == 1 (all from
// attn_decode_common.h).  What differs is how a chunk is read:
//
// Loads: a key row of D bytes is read by Dp/16 adjacent lanes, 16 bytes
// each, so one wave instruction covers 64/(Dp/16) whole rows, twice the
// rows of the bf16 kernel, and the four waves of a round 4x that.  A chunk
// is 2 / 4 / 8 rounds at Dp 64 / 128 / 256 and all of them are in flight
// before the first wait: the whole K (then V) of the chunk in one batch, as
// many bytes per lane as the bf16 kernel keeps in flight.  The row's k_scale
// is loaded with its bytes, by every lane of the row's group (one address);
// v_scale is loaded once per row by the thread that owns the row's
// probability.  Rows at or past len_b and columns at or past D are never
// loaded, their scales included.
//
// Math, all fp32: bytes are widened with v_cvt_pk_f32_fp8,
//   s = ((q . k8_row) * k_scale[row]) * scale (+ slope * (row - (len-1)))
//   p = exp(s - m_c), l_c = sum p (unscaled), then p * v_scale[row] is what
//   multiplies the v8 bytes: acc += (p * v_scale[row]) * v8_row.
// P is not rounded and o is rounded to bf16 once.  A row whose scale is NaN
// (kv_cache_append stores NaN for a row that held a NaN or an Inf) gives a
// NaN score and so a NaN output for its slot: nothing is clamped.
//
// Bit invariance, as for the bf16 kernel: which lane adds what in which
// order (lane groups, then waves, then chunks in ascending order) is a
// function of the position inside the chunk and of len_b alone, and CHUNK
// depends on the head-dim instantiation only.  So o[b, h] and lse[b, h]
// depend on that slot's q, its first len_b rows of k8, k_scale, v8 and
// v_scale, len_b, D, scale and the slope, and not on B, H, Skv, what lies
// past len_b, or the other slots.  A slot of length 0 gives o = 0 and
// lse = -inf.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage), partial
// kernel at Dp 64 / 128 / 256, the same with and without ALiBi: 50 / 64 / 88
// VGPRs, 8 / 8 / 5 waves per SIMD, 1552 / 2576 / 4624 B of LDS, no scratch.
// The combine kernel as instantiated here: 10 VGPRs, 8 waves per SIMD, no
// LDS, no scratch.
#include "attn_decode_common.h"
#include "launchers.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16 e4m3 bytes -> 16 floats, in memory order
__device__ __forceinline__ void unpack_e4m3x16(u32x4 x, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// Dp: head dim padded to 64/128/256; CH: keys per chunk; AL: ALiBi bias.
// st: q and o in bf16 elements, k8 and v8 in bytes.  ws as in
// attention_decode.hip; unused when gridDim.x == 1.
template <int Dp, int CH, bool AL>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_fp8_partial_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ k8,
    const float* __restrict__ k_scale, const unsigned char* __restrict__ v8,
    const float* __restrict__ v_scale, short* __restrict__ o,
    float* __restrict__ lse_out, float* __restrict__ ws, int H, int Skv,
    int D, float scale, const float* __restrict__ alibi,
    const int* __restrict__ kv_lens, AttnStrides st, ScaleStrides sc) {
  constexpr int LPR = Dp / 16;           // lanes per key row
  constexpr int RPI = 64 / LPR;          // rows per wave load instruction
  constexpr int RPR = DEC_WAVES * RPI;   // rows per workgroup round
  constexpr int U = CH / RPR;            // rounds: all of them in flight
  static_assert(Dp <= DEC_THREADS && CH % RPR == 0 && U <= 8 &&
                    CH <= DEC_THREADS,
                "a chunk is at most 8 whole rounds and one row per thread");

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
  const int dg = (lane % LPR) * 16;    // this lane's 16 head-dim columns
  const bool col_ok = dg < D;          // D % 16 == 0: then dg + 16 <= D

  __shared__ float s_lds[CH];          // scores, then p * v_scale
  __shared__ float red[DEC_WAVES][Dp];
  __shared__ float rbuf[DEC_WAVES];

  float qf[16];
  {
    bf16x8 q0 = {0, 0, 0, 0, 0, 0, 0, 0}, q1 = q0;
    if (col_ok) {
      const short* qp = q + batch * st.qb + head * st.qh + dg;
      q0 = *reinterpret_cast<const bf16x8*>(qp);
      q1 = *reinterpret_cast<const bf16x8*>(qp + 8);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qf[j] = bf2f(q0[j]);
      qf[8 + j] = bf2f(q1[j]);
    }
  }
  const unsigned char* kp = k8 + batch * st.kb + head * st.kh +
                            (int64_t)start * st.ks + dg;
  const unsigned char* vp = v8 + batch * st.vb + head * st.vh +
                            (int64_t)start * st.vs + dg;
  const float* ksp = k_scale + batch * sc.kb + head * sc.kh +
                     (int64_t)start * sc.ks;
  const float* vsp = v_scale + batch * sc.vb + head * sc.vh +
                     (int64_t)start * sc.vs;
  const float al_slope = AL ? alibi[head] : 0.f;
  const u32x4 zero = {0u, 0u, 0u, 0u};

  // ---- scores: row = u * RPR + wave * RPI + grp ----
  float wmax = -INFINITY;
  {
    u32x4 kr[U];
    float ksc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = u * RPR + wave * RPI + grp;
      kr[u] = zero;
      ksc[u] = 0.f;
      if (row < n) {
        ksc[u] = ksp[(int64_t)row * sc.ks];
        if (col_ok)
          kr[u] = *reinterpret_cast<const u32x4*>(kp + (int64_t)row * st.ks);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = u * RPR + wave * RPI + grp;
      float kf[16];
      unpack_e4m3x16(kr[u], kf);
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) dot = fmaf(kf[j], qf[j], dot);
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) dot += __shfl_xor(dot, off, 64);
      float s = (dot * ksc[u]) * scale;
      if (AL)
        s = fmaf(al_slope, (float)(start + row - (len - 1)), s);
      s = (row < n) ? s : -INFINITY;
      if (dg == 0) s_lds[row] = s;
      wmax = fmaxf(wmax, s);
    }
  }
  // fmaxf drops a NaN score; its p below is NaN, which the FMAs into acc
  // and into the combine keep, so the slot's o is NaN
  const float m = block_reduce_max(wmax, rbuf);  // also publishes s_lds

  // ---- probabilities, fp32; what is kept is p * v_scale[row] ----
  float lpart = 0.f;
  {
    const int t = threadIdx.x;
    if (t < CH) {
      float p = 0.f, pv = 0.f;
      if (t < n) {
        const float s = s_lds[t];
        p = (s == -INFINITY) ? 0.f : __expf(s - m);
        pv = p * vsp[(int64_t)t * sc.vs];
      }
      s_lds[t] = pv;
      lpart = p;
    }
  }
  const float l = block_reduce_sum(lpart, rbuf);  // also publishes pv

  // ---- acc = sum (p * v_scale) v8, same row -> lane map ----
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  {
    u32x4 vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = u * RPR + wave * RPI + grp;
      vr[u] = zero;
      if (row < n && col_ok)
        vr[u] = *reinterpret_cast<const u32x4*>(vp + (int64_t)row * st.vs);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = u * RPR + wave * RPI + grp;
      const float p = s_lds[row];  // 0 for a dead row, whose v8 is 0 too
      float vf[16];
      unpack_e4m3x16(vr[u], vf);
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
    }
  }
  // the wave's row groups, then the four waves, in a fixed order
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) red[wave][dg + j] = acc[j];
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

extern "C" {

hipError_t launch_attn_decode_fp8(const void* q, const void* k8,
                                  const float* k_scale, const void* v8,
                                  const float* v_scale, void* o, float* lse,
                                  float* ws, int64_t B, int64_t H,
                                  int64_t Skv, int64_t D, float scale,
                                  const float* alibi, const int* kv_lens,
                                  const int64_t* strides,
                                  hipStream_t stream) {
  const AttnStrides st = attn_strides(strides);
  const ScaleStrides sc = {strides[12], strides[13], strides[14],
                           strides[15], strides[16], strides[17]};
  if (D <= 0 || D % 16 != 0 || D > 256 || B * H > 65535)
    return hipErrorInvalidValue;
#define DEC8_LAUNCH(DP, ALB)                                               \
  do {                                                                     \
    constexpr int CH = DecodeChunk<DP>::value;                             \
    const int64_t n_chunks = Skv > 0 ? ceil_div(Skv, CH) : 1;              \
    dim3 grid((uint32_t)n_chunks, (uint32_t)(B * H));                      \
    attn_decode_fp8_partial_kernel<DP, CH, ALB>                            \
        <<<grid, dim3(DEC_THREADS), 0, stream>>>(                          \
            (const short*)q, (const unsigned char*)k8, k_scale,            \
            (const unsigned char*)v8, v_scale, (short*)o, lse, ws, (int)H, \
            (int)Skv, (int)D, scale, alibi, kv_lens, st, sc);              \
    if (n_chunks > 1)                                                      \
      attn_decode_combine_kernel<CH>                                       \
          <<<dim3((uint32_t)(B * H)), dim3(DEC_THREADS), 0, stream>>>(     \
              ws, (short*)o, lse, (int)H, (int)Skv, (int)D, (int)n_chunks, \
              kv_lens, st);                                                \
  } while (0)
#define DEC8_DISPATCH(DP)                                                  \
  do {                                                                     \
    if (alibi) DEC8_LAUNCH(DP, true);                                      \
    else DEC8_LAUNCH(DP, false);                                           \
  } while (0)
  if (D <= 64) {
    DEC8_DISPATCH(64);
  } else if (D <= 128) {
    DEC8_DISPATCH(128);
  } else {
    DEC8_DISPATCH(256);
  }
#undef DEC8_DISPATCH
#undef DEC8_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
