// Flash attention BACKWARD (bf16, causal/full) for gfx950: deterministic
// two-kernel split (no atomics) — a dq kernel over q blocks and a dk/dv
// kernel over kv blocks, each recomputing P from (q, k, lse).
// delta = rowsum(dO * O) is precomputed by attn_bwd_preprocess_kernel.
//
// Both kernels keep P and dS in registers.  The first products are oriented
// so that the later products sum over their ROW index: the f32 accumulator
// tile (rows in the 4 registers, columns on the lanes) is rounded to bf16
// and is directly the A operand of the next MFMA.  Two 16-row sub-tiles
// make one k = 32 step, whose k order is permuted: element j of lane group
// h (= lane >> 4) is row 16*(j>>2) + 4*h + (j&3) of the 32-row step.  The
// other operand is read in that same order with ds_read_b64_tr_b16 from
// the one row-major LDS image of the staged tile, so no transposed second
// image and no P/dS round trip through LDS exist.
//
// Head dim: DK is the staged row width (64, 80, 96 or 128).  D = 80 gets
// rows of exactly 80 elements and 5 output d-tiles.  Its contraction over d
// is two k = 32 steps plus a third whose upper 16 k-slots are zero in the
// register-side operand.  (mfma_f32_16x16x16bf16_1k for that step passed
// the exact-data test in most instantiations but gave wrong and run-to-run
// different dq values in others on MI355X, whether it ended or began the
// accumulation chain; the zero-padded 16x16x32 step is exact everywhere
// and costs 3 % of the backward's time.)  Other D pad up to the next DK
// with zeros.
//
// A wave owns RW sets of 16 rows (RW = 2 for DK <= 96): every LDS fragment
// it reads feeds RW MFMAs, which takes the loop off the LDS-bandwidth limit
// of one read per MFMA.  A block is 128 rows either way (4 waves x 32 or
// 8 waves x 16).
//
// LDS rows are RS = DK (+16 if DK is a multiple of 32) elements, so a row is
// an odd multiple of 8 dwords.  By the bank rule (bank = dword mod 64):
//   - ds_read_b128 row fragments: the 8 distinct rows mod 8 of a 16-lane
//     group land on 8 distinct 8-dword slots, the two lane>>4 values of the
//     group on its two 4-dword halves — conflict-free;
//   - ds_read_b64_tr_b16: a 32-lane half covers 8 consecutive rows x 8
//     dwords, again 8 distinct slots — conflict-free;
//   - the tail step's ds_read_b128 (DK = 80 only) reads columns
//     64 + 8*(lane>>4 & 1): lane groups 0/2 and 1/3 share addresses
//     (broadcast), the rest is as for the other row fragments.
//
// The staged tiles are double-buffered: global loads for tile t+1 issue
// before the MFMAs of tile t, are written to the other buffer after them,
// and one barrier per tile separates the two.
//
// MFMA fragment layouts (verified by the mfma_probe and exact-data tests):
//   16x16x32: A[m = lane&15][k = 8*(lane>>4) + j], B[k = same][n = lane&15]
//   C/D     : [m = 4*(lane>>4) + reg][n = lane&15]
#include <climits>

#include "attn_tile.h"
#include "common.h"
#include "launchers.h"

// All tensors logically [B, H, S, D] with arbitrary B/H/S strides and a
// contiguous D (so the packed qkv/dqkv layouts feed the kernels directly).
struct AttnBwdStrides {
  int64_t qb, qh, qs;
  int64_t kb, kh, ks;
  int64_t vb, vh, vs;
  int64_t dob, doh, dos;
  int64_t dqb, dqh, dqs;
  int64_t dkb, dkh, dks;
  int64_t dvb, dvh, dvs;
};

// s: the launcher's 24-entry array, q(3) k(3) v(3) do(3) dq(3) dk(3) dv(3)
// o(3); the o strides s[21..23] go to the preprocess kernel only
static AttnBwdStrides attn_bwd_strides(const int64_t* s) {
  return {s[0],  s[1],  s[2],  s[3],  s[4],  s[5],  s[6],
          s[7],  s[8],  s[9],  s[10], s[11], s[12], s[13],
          s[14], s[15], s[16], s[17], s[18], s[19], s[20]};
}

__global__ void attn_bwd_preprocess_kernel(const short* __restrict__ dout,
                                           const short* __restrict__ o,
                                           float* __restrict__ delta,
                                           int64_t rows, int H, int S, int D,
                                           int64_t dob, int64_t doh,
                                           int64_t dos, int64_t ob,
                                           int64_t oh, int64_t os) {
  // 16 lanes x bf16x8 per row, 4 rows per wave (the one-wave-per-row
  // version left 44/64 lanes idle at D=80 and ran 6.7x off roofline)
  int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4);
  if (row >= rows) return;
  int lane16 = threadIdx.x & 15;
  int64_t sidx = row % S, h = (row / S) % H, b = row / ((int64_t)S * H);
  const short* dr = dout + b * dob + h * doh + sidx * dos;
  const short* orow = o + b * ob + h * oh + sidx * os;
  float s = 0.f;
  for (int i = lane16 * 8; i + 8 <= D; i += 16 * 8) {
    bf16x8 dv = *reinterpret_cast<const bf16x8*>(dr + i);
    bf16x8 ov = *reinterpret_cast<const bf16x8*>(orow + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bf2f(dv[j]) * bf2f(ov[j]);
  }
  // D not a multiple of 8: scalar tail on lane 0
  if (lane16 == 0)
    for (int i = (D / 8) * 8; i < D; ++i)
      s += bf2f(dr[i]) * bf2f(orow[i]);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane16 == 0) delta[row] = s;
}

// ---------------------------------------------------------------- dq kernel
// Block: NW waves x RW x 16 q rows = 128 q rows; loops kv tiles of 64.
//   S^T  = K Q^T        (A = K rows from k_lds, B = Q regs)
//   P^T  = exp(S^T*scale - lse[q])
//   dP^T = V dO^T       (A = V rows from v_lds, B = dO regs)
//   dS^T = P^T*(dP^T - delta[q])*scale        (kv in registers, q on lanes)
//   dQ  += dS K         (A = dS^T accumulator as bf16, B = k_lds transposed
//                        read)
template <int DK, int RW, int NW, bool AL = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dq_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dq, int H, int S, int Skv, int D, float scale,
    int causal, const float* __restrict__ alibi, AttnBwdStrides st) {
  using T = AttnTile<DK>;
  constexpr int NT = 4;               // 64 kv per tile = 4 sub-tiles of 16
  constexpr int NTHR = NW * 64;
  constexpr int WROWS = 16 * RW;      // q rows per wave
  constexpr int ROWS = NW * WROWS;    // q rows per block
  constexpr int G_IT = (T::GROUPS + NTHR - 1) / NTHR;

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
  const short* dop = dout + batch * st.dob + head * st.doh;
  short* dqp = dq + batch * st.dqb + head * st.dqh;
  const int q_row0 = qb * ROWS + wave * WROWS;

  __shared__ __attribute__((aligned(16))) short k_lds[2][64][T::RS];
  __shared__ __attribute__((aligned(16))) short v_lds[2][64][T::RS];

  // this lane's q rows (columns of S^T): fragments and row constants;
  // lse is pre-multiplied by log2(e) for the exp2 below
  RowFrag<DK> q_frag[RW], do_frag[RW];
  float lse2_q[RW], delta_q[RW];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    int my_q = q_row0 + 16 * rw + lo;
    int row = min(my_q, S - 1);
    load_row_frag<DK>(q_frag[rw], qp + (int64_t)row * st.qs, hi, D);
    load_row_frag<DK>(do_frag[rw], dop + (int64_t)row * st.dos, hi, D);
    lse2_q[rw] =
        (my_q < S) ? lse[(int64_t)bh * S + my_q] * ATTN_LOG2E : 0.f;
    delta_q[rw] = (my_q < S) ? delta[(int64_t)bh * S + my_q] : 0.f;
  }
  const float scale2 = scale * ATTN_LOG2E;
  const float al_slope2 = AL ? alibi[bh % H] * ATTN_LOG2E : 0.f;

  // first masked kv of this lane's q rows: Skv, q + 1 under the causal
  // mask, 0 (nothing valid) for a q row past S
  int kv_end[RW];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    int my_q = q_row0 + 16 * rw + lo;
    kv_end[rw] = (my_q >= S) ? 0 : (causal ? min(my_q + 1, Skv) : Skv);
  }

  f32x4 dq_acc[RW][T::DT];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw)
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt)
      dq_acc[rw][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kv_limit = causal ? min(Skv, qb * ROWS + ROWS) : Skv;
  const int n_tiles = (kv_limit + 63) / 64;

  // staging: bf16x8 group g = threadIdx.x + it*NTHR of the 64-row tile
  bf16x8 kreg[G_IT], vreg[G_IT];
  auto issue_loads = [&](int tile) {
#pragma unroll
    for (int it = 0; it < G_IT; ++it) {
      int g = threadIdx.x + it * NTHR;
      int row = g / T::GPR, dg = (g % T::GPR) * 8;
      int src = tile * 64 + row;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[it] = z;
      vreg[it] = z;
      if (g < T::GROUPS && src < Skv && dg + 8 <= D) {
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
    const int kvb = ti * 64;
    const int cur = ti & 1;
    const bool more = ti + 1 < n_tiles;
    if (more) issue_loads(ti + 1);  // lands under the MFMAs below

    // causal: kv tiles entirely above this wave's q rows are masked out
    // (wave-uniform, so EXEC stays all ones around the transposed reads).
    // One code path updates the accumulators: a second one (say, without
    // the mask) makes the compiler keep two copies of them.
    if (!(causal && kvb > q_row0 + WROWS - 1)) {
      __builtin_amdgcn_s_setprio(1);
      u32x4 ds_a[RW][2];  // dS^T as the A operand of the two k = 32 steps
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 sa[RW], da[RW];
#pragma unroll
        for (int rw = 0; rw < RW; ++rw) {
          sa[rw] = f32x4{0.f, 0.f, 0.f, 0.f};
          da[rw] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        rows_x_frags<DK, RW>(&k_lds[cur][nt * 16 + lo][0], hi, q_frag, sa);
        rows_x_frags<DK, RW>(&v_lds[cur][nt * 16 + lo][0], hi, do_frag, da);
        // C: row = kv (nt*16 + hi*4 + r), col = q (lo)
#pragma unroll
        for (int rw = 0; rw < RW; ++rw) {
          const int my_q = q_row0 + 16 * rw + lo;
          float ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int kv_idx = kvb + nt * 16 + hi * 4 + r;
            float x = fmaf(sa[rw][r], scale2, -lse2_q[rw]);
            if (AL) x = fmaf(al_slope2, (float)(kv_idx - my_q), x);
            float pv = __builtin_amdgcn_exp2f(x);
            // valid iff kv_idx < kv_end, the lane's first masked kv
            pv = (kv_idx < kv_end[rw]) ? pv : 0.f;
            ds[r] = pv * (da[rw][r] - delta_q[rw]) * scale;
          }
          ds_a[rw][nt >> 1][2 * (nt & 1)] = pack_bf16(ds[0], ds[1]);
          ds_a[rw][nt >> 1][2 * (nt & 1) + 1] = pack_bf16(ds[2], ds[3]);
        }
      }
      // dQ += dS @ K, K read column-wise from the row-major image
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 a[RW];
#pragma unroll
        for (int rw = 0; rw < RW; ++rw) a[rw] = ds_a[rw][s];
        frags_x_cols<DK, RW>(a, &k_lds[cur][32 * s][0], lo, hi, dq_acc);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (more) write_tile(1 - cur);
    __syncthreads();
  }

#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int q_idx = q_row0 + 16 * rw + hi * 4 + r;
      if (q_idx >= S) continue;
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        int col = dt * 16 + lo;
        if (col < D)
          dqp[(int64_t)q_idx * st.dqs + col] = f2bf(dq_acc[rw][dt][r]);
      }
    }
  }
}

// ------------------------------------------------------------- dk/dv kernel
// Block: NW waves x RW x 16 kv rows = 128 kv rows; loops q tiles of 64
// (from the diagonal for causal).
//   S  = Q K^T          (A = Q rows from q_lds, B = K regs)
//   P  = exp(S*scale - lse[q])
//   dP = dO V^T         (A = dO rows from do_lds, B = V regs)
//   dS = P*(dP - delta[q])*scale              (q in registers, kv on lanes)
//   dV += P^T dO        (A = P accumulator as bf16, B = do_lds transposed
//                        read)
//   dK += dS^T Q        (A = dS accumulator as bf16, B = q_lds transposed
//                        read)
template <int DK, int RW, int NW, bool AL = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dkv_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dk, short* __restrict__ dv, int H, int S, int Skv,
    int D, float scale, int causal, const float* __restrict__ alibi,
    AttnBwdStrides st) {
  using T = AttnTile<DK>;
  constexpr int NT = 4;               // 64 q per tile = 4 sub-tiles of 16
  constexpr int NTHR = NW * 64;
  constexpr int WROWS = 16 * RW;      // kv rows per wave
  constexpr int ROWS = NW * WROWS;    // kv rows per block
  constexpr int G_IT = (T::GROUPS + NTHR - 1) / NTHR;
  static_assert(NTHR >= 64, "threads 0..63 stage lse/delta");

  const int flat_ = xcd_swizzle(
      (int)(blockIdx.y * gridDim.x + blockIdx.x),
      (int)(gridDim.x * gridDim.y));
  const int kvb_idx = flat_ % (int)gridDim.x;
  const int bh = flat_ / (int)gridDim.x;
  const int batch = bh / H, head = bh % H;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int lo = lane & 15, hi = lane >> 4;

  const short* qp = q + batch * st.qb + head * st.qh;
  const short* kp = k + batch * st.kb + head * st.kh;
  const short* vp = v + batch * st.vb + head * st.vh;
  const short* dop = dout + batch * st.dob + head * st.doh;
  short* dkp = dk + batch * st.dkb + head * st.dkh;
  short* dvp = dv + batch * st.dvb + head * st.dvh;
  const int kv_row0 = kvb_idx * ROWS + wave * WROWS;
  const float scale2 = scale * ATTN_LOG2E;
  const float al_slope2 = AL ? alibi[bh % H] * ATTN_LOG2E : 0.f;

  __shared__ __attribute__((aligned(16))) short q_lds[2][64][T::RS];
  __shared__ __attribute__((aligned(16))) short do_lds[2][64][T::RS];
  // per q row: lse * log2(e) and delta
  __shared__ __attribute__((aligned(16))) float lse2_lds[2][64];
  __shared__ __attribute__((aligned(16))) float delta_lds[2][64];

  // this lane's kv rows (columns of S)
  RowFrag<DK> k_frag[RW], v_frag[RW];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    int row = min(kv_row0 + 16 * rw + lo, Skv - 1);
    load_row_frag<DK>(k_frag[rw], kp + (int64_t)row * st.ks, hi, D);
    load_row_frag<DK>(v_frag[rw], vp + (int64_t)row * st.vs, hi, D);
  }

  // first unmasked q of this lane's kv rows: kv under the causal mask, 0
  // without it, none for a kv row past Skv.  q rows past S need no mask:
  // they are staged as zeros with lse = delta = 0, so P is finite and
  // multiplies a zero dO row, and dS is zero.
  int q_lo[RW];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
    int my_kv = kv_row0 + 16 * rw + lo;
    q_lo[rw] = (my_kv >= Skv) ? INT_MAX : (causal ? my_kv : 0);
  }

  f32x4 dk_acc[RW][T::DT], dv_acc[RW][T::DT];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw)
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) {
      dk_acc[rw][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv_acc[rw][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  const int q_start = causal ? kvb_idx * ROWS / 64 * 64 : 0;
  const int n_tiles = (S - q_start + 63) / 64;

  // staging: bf16x8 group g = threadIdx.x + it*NTHR of the 64-row tile;
  // threads 0..63 also carry lse/delta of one q row each
  bf16x8 qreg[G_IT], doreg[G_IT];
  float lse_reg, delta_reg;
  auto issue_loads = [&](int tile) {
    int qb0 = q_start + tile * 64;
#pragma unroll
    for (int it = 0; it < G_IT; ++it) {
      int g = threadIdx.x + it * NTHR;
      int row = g / T::GPR, dg = (g % T::GPR) * 8;
      int src = qb0 + row;
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      qreg[it] = z;
      doreg[it] = z;
      if (g < T::GROUPS && src < S && dg + 8 <= D) {
        qreg[it] = *reinterpret_cast<const bf16x8*>(
            qp + (int64_t)src * st.qs + dg);
        doreg[it] = *reinterpret_cast<const bf16x8*>(
            dop + (int64_t)src * st.dos + dg);
      }
    }
    lse_reg = delta_reg = 0.f;
    if (threadIdx.x < 64) {
      int src = qb0 + threadIdx.x;
      if (src < S) {
        lse_reg = lse[(int64_t)bh * S + src];
        delta_reg = delta[(int64_t)bh * S + src];
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int it = 0; it < G_IT; ++it) {
      int g = threadIdx.x + it * NTHR;
      int row = g / T::GPR, dg = (g % T::GPR) * 8;
      if (g < T::GROUPS) {
        *reinterpret_cast<bf16x8*>(&q_lds[buf][row][dg]) = qreg[it];
        *reinterpret_cast<bf16x8*>(&do_lds[buf][row][dg]) = doreg[it];
      }
    }
    if (threadIdx.x < 64) {
      lse2_lds[buf][threadIdx.x] = lse_reg * ATTN_LOG2E;
      delta_lds[buf][threadIdx.x] = delta_reg;
    }
  };

  if (n_tiles > 0) {
    issue_loads(0);
    write_tile(0);
    __syncthreads();
  }

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int qb0 = q_start + ti * 64;
    const int cur = ti & 1;
    const bool more = ti + 1 < n_tiles;
    if (more) issue_loads(ti + 1);  // lands under the MFMAs below

    // causal: q tiles entirely before this wave's kv rows are masked out
    // (wave-uniform, so EXEC stays all ones around the transposed reads).
    // One code path updates the accumulators: a second one (say, without
    // the mask) makes the compiler keep two copies of them.
    if (!(causal && qb0 + 63 < kv_row0)) {
      __builtin_amdgcn_s_setprio(1);
      // one k = 32 step (two 16-row q sub-tiles) at a time, so only one
      // step's P and dS fragments are live
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 p_a[RW], ds_a[RW];  // P, dS as the A operands of this step
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int nt = 2 * s + h;
          f32x4 sa[RW], da[RW];
#pragma unroll
          for (int rw = 0; rw < RW; ++rw) {
            sa[rw] = f32x4{0.f, 0.f, 0.f, 0.f};
            da[rw] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          rows_x_frags<DK, RW>(&q_lds[cur][nt * 16 + lo][0], hi, k_frag, sa);
          rows_x_frags<DK, RW>(&do_lds[cur][nt * 16 + lo][0], hi, v_frag,
                               da);
          // C: row = q (nt*16 + hi*4 + r), col = kv (lo); the row
          // constants are one broadcast 16-byte read each
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(
              &lse2_lds[cur][nt * 16 + hi * 4]);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(
              &delta_lds[cur][nt * 16 + hi * 4]);
#pragma unroll
          for (int rw = 0; rw < RW; ++rw) {
            const int my_kv = kv_row0 + 16 * rw + lo;
            float pv[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int q_idx = qb0 + nt * 16 + hi * 4 + r;
              float x = fmaf(sa[rw][r], scale2, -l4[r]);
              if (AL) x = fmaf(al_slope2, (float)(my_kv - q_idx), x);
              pv[r] = __builtin_amdgcn_exp2f(x);
              pv[r] = (q_idx >= q_lo[rw]) ? pv[r] : 0.f;
              ds[r] = pv[r] * (da[rw][r] - d4[r]) * scale;
            }
            p_a[rw][2 * h] = pack_bf16(pv[0], pv[1]);
            p_a[rw][2 * h + 1] = pack_bf16(pv[2], pv[3]);
            ds_a[rw][2 * h] = pack_bf16(ds[0], ds[1]);
            ds_a[rw][2 * h + 1] = pack_bf16(ds[2], ds[3]);
          }
        }
        // dV += P^T @ dO and dK += dS^T @ Q, dO and Q read column-wise
        // from their row-major images
        frags_x_cols<DK, RW>(p_a, &do_lds[cur][32 * s][0], lo, hi, dv_acc);
        frags_x_cols<DK, RW>(ds_a, &q_lds[cur][32 * s][0], lo, hi, dk_acc);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (more) write_tile(1 - cur);
    __syncthreads();
  }

#pragma unroll
  for (int rw = 0; rw < RW; ++rw) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int kv_idx = kv_row0 + 16 * rw + hi * 4 + r;
      if (kv_idx >= Skv) continue;
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        int col = dt * 16 + lo;
        if (col < D) {
          dkp[(int64_t)kv_idx * st.dks + col] = f2bf(dk_acc[rw][dt][r]);
          dvp[(int64_t)kv_idx * st.dvs + col] = f2bf(dv_acc[rw][dt][r]);
        }
      }
    }
  }
}

extern "C" {

hipError_t launch_attn_bwd(const void* q, const void* k, const void* v,
                           const void* o, const void* dout,
                           const float* lse, float* delta_ws, void* dq,
                           void* dk, void* dv, int64_t B, int64_t H,
                           int64_t S, int64_t Skv, int64_t D, float scale,
                           int causal, const float* alibi,
                           const int64_t* strides, hipStream_t stream) {
  // reject before anything is enqueued
  if (D > 128) return hipErrorInvalidValue;
  const AttnBwdStrides st = attn_bwd_strides(strides);
  int64_t rows = B * H * S;
  {
    dim3 block(256);
    dim3 grid((uint32_t)ceil_div(rows, 16));  // 16 rows per 256-thr block
    attn_bwd_preprocess_kernel<<<grid, block, 0, stream>>>(
        (const short*)dout, (const short*)o, delta_ws, rows, (int)H, (int)S,
        (int)D, st.dob, st.doh, st.dos, strides[21], strides[22],
        strides[23]);
  }
  // dq and dkv are independent (disjoint outputs, shared read-only
  // inputs) — launching them on two streams lets the CU scheduler
  // co-resident them and fill the SIMDs.
  static hipStream_t side_stream = nullptr;
  static hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  if (side_stream == nullptr) {
    (void)hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking);
    (void)hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&ev_join, hipEventDisableTiming);
  }
  (void)hipEventRecord(ev_fork, stream);
  (void)hipStreamWaitEvent(side_stream, ev_fork, 0);
  constexpr int BLOCK_ROWS = 128;  // NW * RW * 16 in every configuration
  dim3 grid_q((uint32_t)ceil_div(S, BLOCK_ROWS), (uint32_t)(B * H));
  dim3 grid_kv((uint32_t)ceil_div(Skv, BLOCK_ROWS), (uint32_t)(B * H));
// RWQ/NWQ: rows-per-wave sets and waves of the dq kernel, RWK/NWK of dkv
#define LAUNCH_BWD_T(DK, RWQ, NWQ, RWK, NWK, ALB)                          \
  do {                                                                     \
    static_assert(NWQ * RWQ * 16 == BLOCK_ROWS, "grid assumes 128 rows");  \
    static_assert(NWK * RWK * 16 == BLOCK_ROWS, "grid assumes 128 rows");  \
    attn_bwd_dq_kernel<DK, RWQ, NWQ, ALB>                                  \
        <<<grid_q, dim3(NWQ * 64), 0, side_stream>>>(                      \
            (const short*)q, (const short*)k, (const short*)v,             \
            (const short*)dout, lse, delta_ws, (short*)dq, (int)H, (int)S, \
            (int)Skv, (int)D, scale, causal, alibi, st);                   \
    attn_bwd_dkv_kernel<DK, RWK, NWK, ALB>                                 \
        <<<grid_kv, dim3(NWK * 64), 0, stream>>>(                          \
            (const short*)q, (const short*)k, (const short*)v,             \
            (const short*)dout, lse, delta_ws, (short*)dk, (short*)dv,     \
            (int)H, (int)S, (int)Skv, (int)D, scale, causal, alibi, st);   \
  } while (0)
#define LAUNCH_BWD(DK, RWQ, NWQ, RWK, NWK)                                 \
  do {                                                                     \
    if (alibi) LAUNCH_BWD_T(DK, RWQ, NWQ, RWK, NWK, true);                 \
    else LAUNCH_BWD_T(DK, RWQ, NWQ, RWK, NWK, false);                      \
  } while (0)
  // 4 waves x 32 rows where two accumulator sets fit 256 registers (two
  // waves per SIMD) without spilling; 8 waves x 16 rows otherwise
  if (D <= 64) {
    LAUNCH_BWD(64, 2, 4, 2, 4);
  } else if (D == 80) {
    // rows of exactly 80: 5 d-tiles, third k step half zero
    LAUNCH_BWD(80, 2, 4, 2, 4);
  } else if (D <= 96) {
    LAUNCH_BWD(96, 2, 4, 1, 8);
  } else {
    LAUNCH_BWD(128, 1, 8, 1, 8);
  }
#undef LAUNCH_BWD
#undef LAUNCH_BWD_T
  (void)hipEventRecord(ev_join, side_stream);
  (void)hipStreamWaitEvent(stream, ev_join, 0);
  return hipGetLastError();
}

}  // extern "C"
