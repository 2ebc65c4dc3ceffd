// What the split-KV decode attention kernels share (attention_decode.hip:
// bf16 cache; attention_decode_fp8.hip: e4m3 cache): the launch geometry, the
// chunk size, the slot length, the one place a row is normalised and the
// combine kernel.  Both partial kernels write the same fp32 workspace, so
// one combine serves both.  The chunk kernel for several query rows
// (attention_chunk.hip) takes the geometry, the chunk size, the slot length
// and the normalisation from here and has a combine of its own.
#pragma once

#include "attn_strides.h"
#include "common.h"

#define DEC_THREADS 256
#define DEC_WAVES (DEC_THREADS / 64)

// Keys per chunk for the instantiation padded to Dp.  A compile-time
// constant per Dp: it must never depend on B, H, Skv or the device, or the
// bit invariance of the kernels is gone.  ops.DECODE_ATTN_CHUNK mirrors it.
template <int Dp>
struct DecodeChunk {
  static constexpr int value = 128;
};

// element strides of the k_scale and v_scale [B, H, Skv] of an e4m3 cache
struct ScaleStrides {
  int64_t kb, kh, ks;
  int64_t vb, vh, vs;
};

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

// One workgroup per (batch, head); thread t owns head-dim column t.
// ws: fp32 [B*H, n_chunks, 2] of (m_c, l_c), then [B*H, n_chunks, D] of
// acc_c, as the partial kernels wrote it.
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
