// Flash attention forward (bf16, causal/full) for gfx950 — MFMA
// 16x16x32_bf16, online softmax, never materializes S x S.
//
// Covers the reference's fused-attention slot (SURVEY.md §2.3 kernel table:
// "batched GEMM + softmax ... fused attention kernel (QK^T->softmax->V)").
//
// Head dims up to 128 run attn_fwd_kernel, built from the tile helpers the
// backward uses (attn_tile.h; the k-order permutation and the LDS bank
// argument are in the header comment of attention_bwd.hip):
//
//   - A block owns 128 q rows of one (batch, head) and loops over kv tiles
//     of 64.  A wave owns RW = 2 sets of 16 q rows (4 waves per block), so
//     every K and V fragment it reads from LDS feeds two MFMAs.
//   - K and V are staged once each, row-major [kv][DK], DK the exact staged
//     row width (64, 80, 96 or 128; other D pad up to the next with zeros).
//     D = 80 stages 80 columns and runs 5 output d-tiles; its contraction
//     over d ends in a k = 32 step whose upper 16 k-slots are zero in Q.
//     Both tiles are double-buffered: global loads for tile t+1 issue before
//     the MFMAs of tile t and are written to the other buffer after them,
//     one barrier per tile.
//   - S^T = K Q^T (A = K rows from LDS, B = Q in registers): a lane holds 16
//     scores of ONE q row per set, so the softmax row reduction is in
//     registers plus two shuffles, and m, l sit on the lanes of their row.
//   - P stays in registers.  O^T = V^T P^T: the S^T accumulator (kv in the 4
//     registers, q on the lanes), after softmax rounded to bf16, is directly
//     the B operand; the A operand V^T is read from the row-major V image
//     with ds_read_b64_tr_b16 in the same permuted k order.  This
//     orientation was chosen over O = P V because the O accumulator then has
//     q on the lanes like the softmax state: alpha and 1/l apply with no
//     cross-lane move, and a lane ends with 4 consecutive d of one q row,
//     which is one 8-byte store per d-tile.
//   - The deferred rescale (threshold 8) is decided per 16-row set.
//   - Masks (causal diagonal, ragged last kv tile, q rows past S), kv_lens
//     and ALiBi run only on the tiles that need them; the choice is
//     wave-uniform, as is every branch around the transposed reads.  Rows
//     past Skv or a slot's length are zero rows in LDS plus masked scores.
//
// Head dims 129..256 run attn_fwd_wide_kernel, the earlier design: 8 waves
// of 16 rows, K tile [64][256] and a transposed V tile in one LDS buffer,
// P re-fragmented through LDS.  No ALiBi or kv_lens there.
//
// The backward pass lives in attention_bwd.hip.
//
// MFMA fragment layouts (verified on hardware by the mfma_probe test,
// kernels in mfma_probe.hip):
//   A (16x32): m = lane&15, k = (lane>>4)*8 + j   (j = 0..7)
//   B (32x16): n = lane&15, k = (lane>>4)*8 + j
//   C/D      : n = lane&15, m = (lane>>4)*4 + reg (f32x4)
#include "attn_strides.h"
#include "attn_tile.h"
#include "common.h"
#include "launchers.h"

#define ATTN_BLOCK_K 64
#define ATTN_BLOCK_Q 128
#define ATTN_WIDE_THREADS 512

// T13 defer-max: skip the O-wide rescale while the max grows by less than
// this (P values then bounded by e^8 = 2981, fine in the f32 accumulator)
#define ATTN_DEFER_THR 8.0f

// ------------------------------------------------------------ D <= 128
// DK: staged row width; RW: 16-row sets per wave; NW: waves per block
// (NW * RW * 16 = 128 q rows); AL: ALiBi bias; VL: per-batch kv lengths
// (varlen decode); o_vec: o rows allow 8-byte stores.
template <int DK, int RW, int NW, bool AL, bool VL>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, int H, int S, int Skv, int D, float scale,
    int causal, const float* __restrict__ alibi,
    const int* __restrict__ kv_lens, int o_vec, AttnStrides st) {
  using T = AttnTile<DK>;
  constexpr int NT = ATTN_BLOCK_K / 16;  // 4 sub-tiles of 16 kv
  constexpr int NTHR = NW * 64;
  constexpr int WROWS = 16 * RW;         // q rows per wave
  constexpr int ROWS = NW * WROWS;       // q rows per block
  constexpr int G_IT = (T::GROUPS + NTHR - 1) / NTHR;
  static_assert(ROWS == ATTN_BLOCK_Q, "grid assumes 128 q rows per block");

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
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int lo = lane & 15, hi = lane >> 4;

  const short* qp = q + batch * st.qb + head * st.qh;
  const short* kp = k + batch * st.kb + head * st.kh;
  const short* vp = v + batch * st.vb + head * st.vh;
  short* op = o + batch * st.ob + head * st.oh;
  const int q_row0 = qb * ROWS + wave * WROWS;

  __shared__ __attribute__((aligned(16))) short k_lds[2][64][T::RS];
  __shared__ __attribute__((aligned(16))) short v_lds[2][64][T::RS];

  // this lane's q rows (columns of S^T)
  RowFrag<DK> q_frag[RW];
  int my_q[RW];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    my_q[rw] = q_row0 + 16 * rw + lo;
    int row = min(my_q[rw], S - 1);
    load_row_frag<DK>(q_frag[rw], qp + (int64_t)row * st.qs, hi, D);
  }

  // softmax state of the lane's q rows, in the units of lse, and
  // O^T: d = 16*dt + 4*hi + reg, q = lo
  float m_state[RW], l_state[RW];
  f32x4 o_acc[RW][T::DT];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    m_state[rw] = -INFINITY;
    l_state[rw] = 0.f;
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt)
      o_acc[rw][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int kv_limit = causal ? min(Skv, qb * ROWS + ROWS) : Skv;
  const int n_tiles = (kv_limit + ATTN_BLOCK_K - 1) / ATTN_BLOCK_K;
  // ALiBi (BLOOM): per-head slope, bias = slope * (kv_pos - q_pos); the
  // q GLOBAL position is my_q + (Skv - S) for cached decode
  // varlen (continuous batching): this batch slot's real kv length;
  // tiles past it are masked per element (Skv stays the tile loop bound)
  const int my_skv = VL ? kv_lens[batch] : Skv;
  const float al_slope = AL ? alibi[bh % H] : 0.f;
  const int al_qoff = my_skv - S;
  // rows at or past the slot's length are never loaded: their scores are
  // masked, but P = 0 times a NaN or Inf left in V there would still be NaN
  const int load_skv = VL ? min(my_skv, Skv) : Skv;

  // staging: bf16x8 group g = threadIdx.x + it*NTHR of the 64-row tile
  bf16x8 kreg[G_IT], vreg[G_IT];
  auto issue_loads = [&](int tile) {
#pragma unroll
    for (int it = 0; it < G_IT; ++it) {
      int g = threadIdx.x + it * NTHR;
      int row = g / T::GPR, dg = (g % T::GPR) * 8;
      int src = tile * ATTN_BLOCK_K + row;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[it] = z;
      vreg[it] = z;
      if (g < T::GROUPS && src < load_skv && dg + 8 <= D) {
        kreg[it] = *reinterpret_cast<const bf16x8*>(
            kp + (int64_t)src * st.ks + dg);
        vreg[it] = *reinterpret_cast<const bf16x8*>(
            vp + (int64_t)src * st.vs + dg);
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int it = 0; it < G_IT; ++it) {
      int g = threadIdx.x + it * NTHR;
      int row = g / T::GPR, dg = (g % T::GPR) * 8;
      if (g < T::GROUPS) {
        *reinterpret_cast<bf16x8*>(&k_lds[buf][row][dg]) = kreg[it];
        *reinterpret_cast<bf16x8*>(&v_lds[buf][row][dg]) = vreg[it];
      }
    }
  };

  if (n_tiles > 0) {
    issue_loads(0);
    write_tile(0);
    __syncthreads();
  }

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int kvb = ti * ATTN_BLOCK_K;
    const int cur = ti & 1;
    const bool more = ti + 1 < n_tiles;
    if (more) issue_loads(ti + 1);  // lands under the MFMAs below

    // causal: kv tiles entirely above this wave's q rows contribute nothing
    // (wave-uniform, so EXEC stays all ones around the transposed reads)
    if (!(causal && kvb > q_row0 + WROWS - 1)) {
      // ---- S^T = K Q^T: s_acc[nt][rw][r] is kv nt*16 + hi*4 + r, q lo ----
      __builtin_amdgcn_s_setprio(1);  // T5: favor the MFMA cluster
      f32x4 s_acc[NT][RW];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int rw = 0; rw < RW; ++rw)
          s_acc[nt][rw] = f32x4{0.f, 0.f, 0.f, 0.f};
        rows_x_frags<DK, RW>(&k_lds[cur][nt * 16 + lo][0], hi, q_frag,
                             s_acc[nt]);
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- scale; bias and masks only where the tile needs them: under
      // ALiBi or kv_lens, on the causal diagonal, on a ragged last kv tile
      // and in a wave with q rows past S ----
      const bool edge = AL || VL || (kvb + ATTN_BLOCK_K > Skv) ||
                        (causal && kvb + ATTN_BLOCK_K - 1 > q_row0) ||
                        (q_row0 + WROWS > S);
      if (edge) {
#pragma unroll
        for (int rw = 0; rw < RW; ++rw)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int kv_idx = kvb + nt * 16 + hi * 4 + r;
              float sv = s_acc[nt][rw][r] * scale;
              if (AL)
                sv = fmaf(al_slope, (float)(kv_idx - my_q[rw] - al_qoff), sv);
              bool masked = (kv_idx >= my_skv) ||
                            (causal && kv_idx > my_q[rw]) || (my_q[rw] >= S);
              s_acc[nt][rw][r] = masked ? -INFINITY : sv;
            }
      } else {
#pragma unroll
        for (int rw = 0; rw < RW; ++rw)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_acc[nt][rw][r] *= scale;
      }

      // ---- online softmax per 16-row set; P^T = exp(S^T - m) as the B
      // operand of the two k = 32 steps ----
      u32x4 p_b[2][RW];
#pragma unroll
      for (int rw = 0; rw < RW; ++rw) {
        // lane-local max over this lane's 16 kv, then across the 4 lane
        // groups that share the q row
        float tile_max = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            tile_max = fmaxf(tile_max, s_acc[nt][rw][r]);
        tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, 64));
        tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));

        // only when some row's max jumps past the threshold does the set
        // rescale and advance m (guide T13)
        if (!__all(tile_max <= m_state[rw] + ATTN_DEFER_THR)) {
          float m_new = fmaxf(m_state[rw], tile_max);
          float alpha = (m_state[rw] == -INFINITY)
                            ? 0.f
                            : __expf(m_state[rw] - m_new);
          m_state[rw] = m_new;
          l_state[rw] *= alpha;
#pragma unroll
          for (int dt = 0; dt < T::DT; ++dt) {
            o_acc[rw][dt][0] *= alpha; o_acc[rw][dt][1] *= alpha;
            o_acc[rw][dt][2] *= alpha; o_acc[rw][dt][3] *= alpha;
          }
        }
        // a row with nothing visible so far has m = -inf and only -inf
        // scores: exp(-inf - 0) = 0 where exp(-inf + inf) would be NaN
        const float m_sub = (m_state[rw] == -INFINITY) ? 0.f : m_state[rw];
        float part = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float pv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[r] = __expf(s_acc[nt][rw][r] - m_sub);
            part += pv[r];
          }
          p_b[nt >> 1][rw][2 * (nt & 1)] = pack_bf16(pv[0], pv[1]);
          p_b[nt >> 1][rw][2 * (nt & 1) + 1] = pack_bf16(pv[2], pv[3]);
        }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        l_state[rw] += part;
      }

      // ---- O^T += V^T P^T, V read column-wise from the row-major image --
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        cols_x_frags<DK, RW>(&v_lds[cur][32 * s][0], lo, hi, p_b[s], o_acc);
      __builtin_amdgcn_s_setprio(0);
    }

    if (more) write_tile(1 - cur);
    __syncthreads();
  }

  // ---- epilogue: lane holds O^T[d = 16*dt + 4*hi + r][q = lo] ----
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    const int q_idx = my_q[rw];
    if (q_idx >= S) continue;
    const float l = l_state[rw];
    const float inv_l = (l > 0.f) ? 1.0f / l : 0.f;
    short* orow = op + (int64_t)q_idx * st.os + hi * 4;
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) {
      if (dt * 16 + hi * 4 >= D) continue;  // D is a multiple of 16
      uint2 pk;
      pk.x = pack_bf16(o_acc[rw][dt][0] * inv_l, o_acc[rw][dt][1] * inv_l);
      pk.y = pack_bf16(o_acc[rw][dt][2] * inv_l, o_acc[rw][dt][3] * inv_l);
      if (o_vec) {
        *reinterpret_cast<uint2*>(orow + dt * 16) = pk;
      } else {
        orow[dt * 16 + 0] = (short)(pk.x & 0xffff);
        orow[dt * 16 + 1] = (short)(pk.x >> 16);
        orow[dt * 16 + 2] = (short)(pk.y & 0xffff);
        orow[dt * 16 + 3] = (short)(pk.y >> 16);
      }
    }
    if (hi == 0 && lse_out != nullptr)
      lse_out[(int64_t)bh * S + q_idx] =
          (l > 0.f) ? m_state[rw] + __logf(l) : -INFINITY;
  }
}

// ------------------------------------------------------ 128 < D <= 256
// Dp = 256: 8 waves x 16 q-rows = 128 q rows per block.  Two buffers do not
// fit in LDS, so the K tile [64][Dp] and the transposed V tile [Dp][64] are
// staged in one buffer (85504 B with the P tile) at two barriers per tile;
// the 16 o_acc f32x4 per lane keep occupancy low.
template <int Dp>
__global__ __launch_bounds__(ATTN_WIDE_THREADS) void attn_fwd_wide_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, int H, int S, int Skv, int D, float scale,
    int causal, AttnStrides st) {
  constexpr int NT = ATTN_WIDE_THREADS;
  constexpr int KSTEPS_QK = Dp / 32;
  constexpr int NTILES = ATTN_BLOCK_K / 16;  // 4
  constexpr int DTILES = Dp / 16;
  constexpr int LP = 4;  // padding: (Dp+LP)*2B stride -> gcd(words,32)=2, 16 distinct banks (LP=8 gave gcd 4 => 2-way conflicts)
  constexpr int NW = NT / 64;                // waves per block
  constexpr int GPR = Dp / 8;                // bf16x8 groups per kv row
  constexpr int TOTAL_G = ATTN_BLOCK_K * GPR;
  constexpr int G_PER_T = (TOTAL_G + NT - 1) / NT;
  static_assert(16 * NW == ATTN_BLOCK_Q, "grid assumes 128 q rows per block");

  // XCD co-location + causal ordering, as in attn_fwd_kernel
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

  __shared__ short k_lds[ATTN_BLOCK_K][Dp + LP];
  __shared__ short vt_lds[Dp][ATTN_BLOCK_K + LP];
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
          if (src < Skv && dg + 8 <= D) {
            kreg[2 * it + u] = *reinterpret_cast<const bf16x8*>(
                kp + (int64_t)src * st.ks + dg);
            vreg[2 * it + u] = *reinterpret_cast<const bf16x8*>(
                vp + (int64_t)src * st.vs + dg);
          }
        }
      }
    }
  };
  auto write_tile = [&]() {
#pragma unroll
    for (int it = 0; it < G_PER_T; ++it) {
      int t = threadIdx.x + it * NT;
      if (t < TOTAL_G / 2) {
        int kvr = (t / GPR) * 2, dg = (t % GPR) * 8;
        *reinterpret_cast<bf16x8*>(&k_lds[kvr][dg]) = kreg[2 * it];
        *reinterpret_cast<bf16x8*>(&k_lds[kvr + 1][dg]) = kreg[2 * it + 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          short2 pr;
          pr.x = vreg[2 * it][j];
          pr.y = vreg[2 * it + 1][j];
          *reinterpret_cast<short2*>(&vt_lds[dg + j][kvr]) = pr;
        }
      }
    }
  };

  auto advance = [&](int ti) {
    if (ti + 1 >= n_tiles) return;
    __syncthreads();      // everyone done reading the buffer
    issue_loads(ti + 1);
    write_tile();
    __syncthreads();
  };

  if (n_tiles > 0) {
    issue_loads(0);
    write_tile();
    __syncthreads();
  }

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int kvb = ti * ATTN_BLOCK_K;

    // causal: tiles entirely above this wave's q rows contribute nothing
    if (causal && kvb > q_row0 + 15) {
      advance(ti);
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
            &k_lds[nt * 16 + lo][ks * 32 + hi * 8]);
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
        bool masked = (kv_idx >= Skv) || (causal && kv_idx > my_q) ||
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
    // only when some lane's max jumps past the threshold does the wave
    // rescale and advance m (guide T13; isolated +5%)
    if (!__all(tile_max <= m_state + ATTN_DEFER_THR)) {
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
            &vt_lds[dt * 16 + lo][ks * 32 + hi * 8]);
        o_acc[dt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, o_acc[dt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    advance(ti);
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
  dim3 grid((uint32_t)ceil_div(S, ATTN_BLOCK_Q), (uint32_t)(B * H));
  // every o row starts on an 8-byte boundary: the epilogue stores 4 bf16
  // at once (2-byte stores otherwise)
  const int o_vec = reinterpret_cast<uintptr_t>(o) % 8 == 0 &&
                    st.ob % 4 == 0 && st.oh % 4 == 0 && st.os % 4 == 0;
#define FWD_LAUNCH(DK, RW, NW, ALB, VLB)                                   \
  attn_fwd_kernel<DK, RW, NW, ALB, VLB><<<grid, dim3(NW * 64), 0, stream>>>( \
      (const short*)q, (const short*)k, (const short*)v, (short*)o, lse,   \
      (int)H, (int)S, (int)Skv, (int)D, scale, causal, alibi, kv_lens,     \
      o_vec, st)
#define FWD_DISPATCH(DK, RW, NW)                                           \
  do {                                                                     \
    if (alibi && kv_lens) FWD_LAUNCH(DK, RW, NW, true, true);              \
    else if (alibi) FWD_LAUNCH(DK, RW, NW, true, false);                   \
    else if (kv_lens) FWD_LAUNCH(DK, RW, NW, false, true);                 \
    else FWD_LAUNCH(DK, RW, NW, false, false);                             \
  } while (0)
  // 4 waves x 32 rows everywhere: at DK = 128 the two accumulator sets, Q
  // and the staging registers still fit the 256 registers of two waves per
  // SIMD without spilling
  if (D <= 64) {
    FWD_DISPATCH(64, 2, 4);
  } else if (D == 80) {
    // rows of exactly 80: 5 d-tiles, third k step half zero
    FWD_DISPATCH(80, 2, 4);
  } else if (D <= 96) {
    FWD_DISPATCH(96, 2, 4);
  } else if (D <= 128) {
    FWD_DISPATCH(128, 2, 4);
  } else if (D <= 256 && !alibi && !kv_lens) {
    // CodeGen-class heads: the plain variant only
    attn_fwd_wide_kernel<256><<<grid, dim3(ATTN_WIDE_THREADS), 0, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)o, lse,
        (int)H, (int)S, (int)Skv, (int)D, scale, causal, st);
  } else {
    return hipErrorInvalidValue;
  }
#undef FWD_DISPATCH
#undef FWD_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
