// Flash attention forward (bf16, causal/full) for gfx950 — MFMA
// 16x16x32_bf16, online softmax, never materializes S x S.
//
// Covers the reference's fused-attention slot (SURVEY.md §2.3 kernel table:
// "batched GEMM + softmax ... fused attention kernel (QK^T->softmax->V)").
//
// Structure: 512 threads = 8 waves per block; block owns 128 q rows of one
// (batch, head); wave owns 16 rows.  K tile [64][Dp] and transposed V tile
// [Dp][64] staged in LDS, shared by all waves — double-buffered for
// Dp <= 128, single-buffered for Dp = 256; per-wave P tile round-trips
// through LDS to re-fragment S (C-layout) into the PV operand.
//
// The backward pass lives in attention_bwd.hip.
//
// MFMA fragment layouts (verified on hardware by the mfma_probe test,
// kernels in mfma_probe.hip):
//   A (16x32): m = lane&15, k = (lane>>4)*8 + j   (j = 0..7)
//   B (32x16): n = lane&15, k = (lane>>4)*8 + j
//   C/D      : n = lane&15, m = (lane>>4)*4 + reg (f32x4)
#include "attn_strides.h"
#include "common.h"
#include "launchers.h"

#define ATTN_BLOCK_K 64
#define ATTN_FWD_THREADS 512

// Dp: head dim padded to the instantiated tile (64/96/128/256); AL: ALiBi
// bias; VL: per-batch kv lengths (varlen decode).
template <int Dp, bool AL = false, bool VL = false>
__global__ __launch_bounds__(ATTN_FWD_THREADS) void attn_fwd_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, int H, int S, int Skv, int D, float scale,
    int causal, const float* __restrict__ alibi,
    const int* __restrict__ kv_lens, AttnStrides st) {
  // 8 waves x 16 q-rows = 128 q rows per block.  For Dp <= 128 the K/V
  // tiles of 64 kv are double-buffered in LDS with register-prefetched
  // staging (loads for tile t+1 issue before computing tile t and land
  // after it — the HBM latency hides under the MFMA/softmax work), one
  // barrier per tile.  Dp = 256 does not fit two buffers in LDS: it stages
  // one buffer (85504 B) and pays two barriers per tile.
  constexpr bool DB = Dp <= 128;
  constexpr int NT = ATTN_FWD_THREADS;
  constexpr int KSTEPS_QK = Dp / 32;
  constexpr int NTILES = ATTN_BLOCK_K / 16;  // 4
  constexpr int DTILES = Dp / 16;
  constexpr int LP = 4;  // padding: (Dp+LP)*2B stride -> gcd(words,32)=2, 16 distinct banks (LP=8 gave gcd 4 => 2-way conflicts)
  constexpr int NW = NT / 64;                // waves per block
  constexpr int GPR = Dp / 8;                // bf16x8 groups per kv row
  constexpr int TOTAL_G = ATTN_BLOCK_K * GPR;
  constexpr int G_PER_T = (TOTAL_G + NT - 1) / NT;

  // XCD co-location + causal ordering: swizzle the flattened id so one
  // XCD owns contiguous (bh, qb) work; within a bh, later q blocks
  // (more kv tiles under causal) go first to avoid a heavy tail
  const int flat_ = xcd_swizzle(
      (int)(blockIdx.y * gridDim.x + blockIdx.x),
      (int)(gridDim.x * gridDim.y));
  const int qb_raw = flat_ % (int)gridDim.x;
  const int qb = causal ? ((int)gridDim.x - 1 - qb_raw) : qb_raw;
  const int bh = flat_ / (int)gridDim.x;
  const int batch = bh / H, head = bh % H;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lo = lane & 15;
  const int hi = lane >> 4;

  const short* qp = q + batch * st.qb + head * st.qh;
  const short* kp = k + batch * st.kb + head * st.kh;
  const short* vp = v + batch * st.vb + head * st.vh;
  short* op = o + batch * st.ob + head * st.oh;
  const int q_row0 = qb * (16 * NW) + wave * 16;

  __shared__ short k_lds[DB ? 2 : 1][ATTN_BLOCK_K][Dp + LP];
  __shared__ short vt_lds[DB ? 2 : 1][Dp][ATTN_BLOCK_K + LP];
  __shared__ short p_lds[NW][16][ATTN_BLOCK_K + LP];

  // ---- Q fragments in registers ----
  bf16x8 q_frag[KSTEPS_QK];
  {
    int row = min(q_row0 + lo, S - 1);
#pragma unroll
    for (int ks = 0; ks < KSTEPS_QK; ++ks) {
      int col = ks * 32 + hi * 8;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      q_frag[ks] = z;
      if (col + 8 <= D)
        q_frag[ks] =
            *reinterpret_cast<const bf16x8*>(qp + (int64_t)row * st.qs + col);
    }
  }

  // Swapped-operand form: the wave computes S^T = K Q^T, so each lane
  // holds 16 S values of ONE q column (q = q_row0 + lo) — the softmax
  // row-reduction is 16 in-register ops + 2 shfl steps across the 4
  // hi-groups (vs 8 serial shfl chains per row in the naive layout).
  // PV becomes O^T = V^T P^T with both operands read contiguously.
  float m_state = -INFINITY, l_state = 0.f;
  f32x4 o_acc[DTILES];  // O^T C-layout: d = hi*4+r (+16*dt), q = lo
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kv_limit =
      causal ? min(Skv, qb * (16 * NW) + 16 * NW) : Skv;
  const int n_tiles = (kv_limit + ATTN_BLOCK_K - 1) / ATTN_BLOCK_K;
  const int my_q = q_row0 + lo;  // this lane's q row
  // ALiBi (BLOOM): per-head slope, bias = slope * (kv_pos - q_pos); the
  // q GLOBAL position is my_q + (Skv - S) for cached decode
  // varlen (continuous batching): this batch slot's real kv length;
  // tiles past it are masked per element (Skv stays the tile loop bound)
  const int my_skv = VL ? kv_lens[batch] : Skv;
  const float al_slope = AL ? alibi[bh % H] : 0.f;
  const int al_qoff = my_skv - S;
  // rows at or past the slot's length are never loaded: their scores are
  // masked, but P = 0 times a NaN or Inf left in V there would still be NaN
  // (compile-time: without VL this is Skv, the original guard)
  const int load_skv = VL ? min(my_skv, Skv) : Skv;

  // staging: load tile -> regs (two kv rows per thread so the V transpose
  // writes pair as b32)
  bf16x8 kreg[2 * G_PER_T], vreg[2 * G_PER_T];
  auto issue_loads = [&](int tile) {
#pragma unroll
    for (int it = 0; it < G_PER_T; ++it) {
      int t = threadIdx.x + it * NT;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[2 * it] = z; kreg[2 * it + 1] = z;
      vreg[2 * it] = z; vreg[2 * it + 1] = z;
      if (t < TOTAL_G / 2) {
        int kvr = (t / GPR) * 2, dg = (t % GPR) * 8;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          int src = tile * ATTN_BLOCK_K + kvr + u;
          if (src < load_skv && dg + 8 <= D) {
            kreg[2 * it + u] = *reinterpret_cast<const bf16x8*>(
                kp + (int64_t)src * st.ks + dg);
            vreg[2 * it + u] = *reinterpret_cast<const bf16x8*>(
                vp + (int64_t)src * st.vs + dg);
          }
        }
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int it = 0; it < G_PER_T; ++it) {
      int t = threadIdx.x + it * NT;
      if (t < TOTAL_G / 2) {
        int kvr = (t / GPR) * 2, dg = (t % GPR) * 8;
        *reinterpret_cast<bf16x8*>(&k_lds[buf][kvr][dg]) = kreg[2 * it];
        *reinterpret_cast<bf16x8*>(&k_lds[buf][kvr + 1][dg]) =
            kreg[2 * it + 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          short2 pr;
          pr.x = vreg[2 * it][j];
          pr.y = vreg[2 * it + 1][j];
          *reinterpret_cast<short2*>(&vt_lds[buf][dg + j][kvr]) = pr;
        }
      }
    }
  };

  auto advance = [&](int ti, int cur) {
    if (ti + 1 >= n_tiles) return;
    if (DB) {
      write_tile(1 - cur);  // waits on the prefetched loads here
      __syncthreads();
    } else {
      __syncthreads();      // everyone done reading buf 0
      issue_loads(ti + 1);
      write_tile(0);
      __syncthreads();
    }
  };

  if (n_tiles > 0) {
    issue_loads(0);
    write_tile(0);
    __syncthreads();
  }

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int kvb = ti * ATTN_BLOCK_K;
    const int cur = DB ? (ti & 1) : 0;
    if (DB && ti + 1 < n_tiles) issue_loads(ti + 1);  // lands under compute

    // causal: tiles entirely above this wave's q rows contribute nothing
    if (causal && kvb > q_row0 + 15) {
      advance(ti, cur);
      continue;
    }

__builtin_amdgcn_s_setprio(1);  // T5: favor the MFMA cluster
    // ---- S^T = K Q^T (A = K tile from LDS, B = Q fragments) ----
    f32x4 s_acc[NTILES];
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSTEPS_QK; ++ks) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &k_lds[cur][nt * 16 + lo][ks * 32 + hi * 8]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, q_frag[ks], acc, 0,
                                                      0, 0);
      }
      s_acc[nt] = acc;
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- mask + scale + lane-local max over this lane's 16 kv ----
    float tile_max = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int kv_idx = kvb + nt * 16 + hi * 4 + r;
        float sv = s_acc[nt][r] * scale;
        if (AL)  // compile-time: the non-ALiBi instantiation is untouched
          sv = fmaf(al_slope, (float)(kv_idx - my_q - al_qoff), sv);
        bool masked = (kv_idx >= my_skv) || (causal && kv_idx > my_q) ||
                      (my_q >= S);
        sv = masked ? -INFINITY : sv;
        s_acc[nt][r] = sv;
        tile_max = fmaxf(tile_max, sv);
      }
    }
    // cross-hi reduce (lanes lo, lo+16, lo+32, lo+48 share q column)
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, 64));
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));

    // ---- online rescale; P^T = exp(S^T - m); sum ----
    // T13 defer-max: skip the O-wide rescale while the max grows by
    // less than THR (P values then bounded by e^THR=2981, fine in f32
    // accum); only when some lane's max jumps past the threshold does
    // the wave rescale and advance m (guide T13; isolated +5%).
    constexpr float DEFER_THR = 8.0f;
    if (!__all(tile_max <= m_state + DEFER_THR)) {
      float m_new = fmaxf(m_state, tile_max);
      float alpha = (m_state == -INFINITY) ? 0.f : __expf(m_state - m_new);
      m_state = m_new;
      l_state *= alpha;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        o_acc[dt][0] *= alpha; o_acc[dt][1] *= alpha;
        o_acc[dt][2] *= alpha; o_acc[dt][3] *= alpha;
      }
    }
    float part = 0.f;
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) {
      bf16x4 pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pval = (s_acc[nt][r] == -INFINITY)
                         ? 0.f
                         : __expf(s_acc[nt][r] - m_state);
        part += pval;
        pk[r] = f2bf(pval);
      }
      // P^T transposed store: p_lds[q][kv], 4 consecutive kv per lane
      // packed into ONE ds_write_b64 (was 4 b16 writes)
      *reinterpret_cast<bf16x4*>(&p_lds[wave][lo][nt * 16 + hi * 4]) = pk;
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    l_state += part;

__builtin_amdgcn_s_setprio(1);  // T5: favor the MFMA cluster
    // ---- O^T += V^T P^T  (A = V^T from vt_lds, B = P^T from p_lds) ----
#pragma unroll
    for (int ks = 0; ks < ATTN_BLOCK_K / 32; ++ks) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &p_lds[wave][lo][ks * 32 + hi * 8]);
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &vt_lds[cur][dt * 16 + lo][ks * 32 + hi * 8]);
        o_acc[dt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, o_acc[dt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    advance(ti, cur);
  }

  // ---- epilogue: lane holds O^T[d = 16*dt + hi*4 + r][q = lo] ----
  {
    int q_idx = q_row0 + lo;
    if (q_idx < S) {
      float inv_l = (l_state > 0.f) ? 1.0f / l_state : 0.f;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int col = dt * 16 + hi * 4 + r;
          if (col < D)
            op[(int64_t)q_idx * st.os + col] = f2bf(o_acc[dt][r] * inv_l);
        }
      }
      if (hi == 0 && lse_out != nullptr)
        lse_out[(int64_t)bh * S + q_idx] =
            (l_state > 0.f) ? m_state + __logf(l_state) : -INFINITY;
    }
  }
}

extern "C" {

hipError_t launch_attn_fwd(const void* q, const void* k, const void* v,
                           void* o, float* lse, int64_t B, int64_t H,
                           int64_t S, int64_t Skv, int64_t D, float scale,
                           int causal, const float* alibi,
                           const int* kv_lens, const int64_t* strides,
                           hipStream_t stream) {
  const AttnStrides st = attn_strides(strides);
  dim3 grid((uint32_t)ceil_div(S, 16 * (ATTN_FWD_THREADS / 64)),
            (uint32_t)(B * H));
  dim3 block(ATTN_FWD_THREADS);
#define FWD_LAUNCH(DP, ALB, VLB)                                           \
  attn_fwd_kernel<DP, ALB, VLB><<<grid, block, 0, stream>>>(               \
      (const short*)q, (const short*)k, (const short*)v, (short*)o, lse,   \
      (int)H, (int)S, (int)Skv, (int)D, scale, causal, alibi, kv_lens, st)
#define FWD_DISPATCH(DP)                                                   \
  do {                                                                     \
    if (alibi && kv_lens) FWD_LAUNCH(DP, true, true);                      \
    else if (alibi) FWD_LAUNCH(DP, true, false);                           \
    else if (kv_lens) FWD_LAUNCH(DP, false, true);                         \
    else FWD_LAUNCH(DP, false, false);                                     \
  } while (0)
  if (D <= 64) {
    FWD_DISPATCH(64);
  } else if (D <= 96) {
    FWD_DISPATCH(96);
  } else if (D <= 128) {
    FWD_DISPATCH(128);
  } else if (D <= 256 && !alibi && !kv_lens) {
    // CodeGen-class heads: the plain variant only, single-buffered K/V;
    // the 16 o_acc f32x4 per lane keep occupancy low
    FWD_LAUNCH(256, false, false);
  } else {
    return hipErrorInvalidValue;
  }
#undef FWD_DISPATCH
#undef FWD_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
