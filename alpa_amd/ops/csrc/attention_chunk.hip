// Split-KV MFMA attention for a chunk of 1..64 query rows over a KV cache
// (bf16 rows, or e4m3 rows with one fp32 scale each) for gfx950: chunked
// prefill, draft-token verification, a multi-token turn on a cached
// conversation.
//
// Semantics: q [B,H,Sq,D]; k, v [B,H,Skv,D] already hold the Sq new rows.
// len_b = clamp(kv_lens[b], 0, Skv) (Skv without lengths) counts them, so
// query row i of slot b sits at position p = len_b - Sq + i and sees keys
// j <= p: a causal mask aligned bottom-right.  ALiBi adds slope_h * (j - p).
// A row with p < 0 sees nothing: o = 0, lse = -inf.
//
// Launches, as attention_decode.hip (flash-decoding, no atomics):
//
//   partial  grid (n_chunks, B*H), 256 threads, CHUNK = DecodeChunk<Dp> keys
//            per workgroup, all QT * 16 query rows.  Writes (m_c, l_c) per
//            row and the unnormalised acc_c[Sq][D] to an fp32 workspace.  A
//            chunk that starts at or past len_b returns before any load or
//            store.
//   combine  grid (B*H, Sq).  Merges chunks 0 .. ceil(len_b/CHUNK)-1 in
//            ascending order and normalises through attn_decode_finish; a
//            row that sees no key of a chunk has m_c = -inf there, weight 0.
//
// With n_chunks == 1 the partial kernel finishes its rows through the same
// attn_decode_finish.
//
// One chunk is one tile: there is no online rescale.  Inside the partial
// kernel (lane = (lo, hi) = (lane & 15, lane >> 4), fragment layouts in the
// header of attention.hip):
//
//   QK^T, split over keys.  Wave w owns keys [32w, 32w + 32) as two 16-key A
//     tiles and computes S^T = K Q^T with mfma_f32_16x16x32_bf16.  Each key
//     is used by one wave only, so K goes from global memory straight into
//     the A fragments, 16 bytes per lane, all of a lane's loads in flight at
//     once, and is never staged.  Q is staged once per workgroup in LDS,
//     [16 QT][Dp + 8], rows past Sq and columns past D as zeros, and read as
//     the B operand.  A lane then holds 8 scores of ONE query row per set:
//     the row maximum is registers plus two shuffles, then one LDS exchange
//     across the four waves.
//   Softmax.  The per-wave row maxima go to LDS; after the barrier
//     m_c = their maximum, p = exp(s - m_c) in fp32.  The per-wave l_c parts
//     go through LDS and are added in wave order.  P is rounded to bf16 once
//     and written to the LDS tile [16 QT][CHUNK + 8], which reuses the bytes
//     of Q (every read of Q is before the first barrier, every write of P
//     after it).
//   PV, split over the head dim.  V is staged once per workgroup, row-major
//     [CHUNK][Dp + 16], dead rows as zeros; its global loads are issued
//     before the QK^T MFMAs and written to LDS after them.  Wave w owns the
//     output d-tiles dt = w, w + 4, ... for all query sets and all 128 keys:
//     O^T = V^T P^T with V^T read through ds_read_b64_tr_b16 (k order: keys
//     4hi..4hi+3 then 16+4hi..16+4hi+3 of a 32-key step, and P is read from
//     LDS in the same order).  No cross-wave reduction of O; d-tiles at or
//     past D and 32-key steps at or past the chunk's live rows are skipped.
//     A lane ends with 4 consecutive d of one query row, the row whose m_c
//     and l_c it already holds.
//   Masks.  The causal edge and the ragged tail touch a chunk only if
//     start + CHUNK - 1 > len_b - Sq; the test is uniform over the workgroup
//     and every other chunk just scales its scores.
//   e4m3.  A lane's 16 bytes of a K row are two k-steps' worth of its
//     k-slots (Q is read from LDS in the matching column order); bytes are
//     widened with v_cvt_pk_f32_fp8 and truncated to bf16, which is exact.
//     k_scale[row] multiplies the fp32 score; V bytes become bf16 while they
//     are staged; v_scale[row] is folded into p in fp32 before the one
//     rounding to bf16 (l_c sums the unscaled p).  A visible row with a NaN
//     scale gives a NaN output, as in attention_decode_fp8.hip.
//
// Rows of k and v at or past len_b and columns at or past D are never
// loaded, and neither are their scales.
//
// Bit invariance: which lane adds what in which order is a function of the
// position inside the chunk, len_b, Sq and the instantiation (Dp, QT), and
// CHUNK depends on Dp only.  So a slot's o and lse do not depend on B, H,
// Skv, what lies past len_b, or the other slots.
//
// Loads are unconditional (see the kernel): guarded ones made the compiler
// branch and wait around each load, and the Dp = 128 bf16 instantiation then
// took 256 VGPRs and spilled.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage), partial
// kernel; with and without ALiBi agree to within 6 registers and the larger
// figure is given.  No scratch in any instantiation.  LDS is dynamic: V,
// max(Q, P) and 512 QT bytes of reductions.
//
//   Dp  QT   bf16: VGPRs  waves/SIMD   e4m3: VGPRs  waves/SIMD   LDS bytes
//   64   1          52        8               69        7           25344
//   64   2          58        8               77        6           30208
//   64   4          90        5               93        5           39936
//  128   1          96        5               88        5           41728
//  128   2          98        4               97        4           46592
//  128   4         126        4              127        4           56320
//  256   1         178        2              142        3           78592
//  256   2         180        2              132        3           87552
//  256   4     192 + 64 AGPRs 2          155 + 64 AGPRs 2          105472
//
// Combine kernel: 10 VGPRs, 8 waves per SIMD, no LDS, no scratch.
#include "attn_decode_common.h"
#include "attn_tile.h"
#include "launchers.h"

// LDS of the partial kernel, in shorts then floats
template <int Dp, int QT>
struct ChunkLds {
  static constexpr int CH = DecodeChunk<Dp>::value;
  static constexpr int QR = 16 * QT;       // staged query rows
  static constexpr int RSV = Dp + 16;      // V row stride (see AttnTile::RS)
  static constexpr int RSQ = Dp + 8;       // Q row stride
  static constexpr int RSP = CH + 8;       // P row stride
  static constexpr int V_SHORTS = CH * RSV;
  static constexpr int QP_SHORTS = QR * (RSQ > RSP ? RSQ : RSP);
  static constexpr int RED_FLOATS = 2 * DEC_WAVES * QR;
  static constexpr size_t BYTES =
      (size_t)(V_SHORTS + QP_SHORTS) * sizeof(short) +
      (size_t)RED_FLOATS * sizeof(float);
  // waves per SIMD to compile for: two workgroups per CU wherever their LDS
  // allows it (the widest case holds 64 accumulator registers per lane)
  static constexpr int WAVES = (Dp == 256 && QT == 4) ? 1 : 2;
  static_assert((RSV / 2) % 16 == 8, "V rows: an odd multiple of 8 dwords");
  static_assert(V_SHORTS % 8 == 0 && QP_SHORTS % 8 == 0, "16-byte sections");
};

// 8 e4m3 bytes (two dwords, memory order) -> 8 bf16, exact
__device__ __forceinline__ uint32_t e4m3_pair_bf16(f32x2 f) {
  return (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u);
}
__device__ __forceinline__ u32x4 e4m3x8_bf16(uint32_t a, uint32_t b) {
  u32x4 r;
  r[0] = e4m3_pair_bf16(__builtin_amdgcn_cvt_pk_f32_fp8(a, false));
  r[1] = e4m3_pair_bf16(__builtin_amdgcn_cvt_pk_f32_fp8(a, true));
  r[2] = e4m3_pair_bf16(__builtin_amdgcn_cvt_pk_f32_fp8(b, false));
  r[3] = e4m3_pair_bf16(__builtin_amdgcn_cvt_pk_f32_fp8(b, true));
  return r;
}

// Dp: head dim padded to 64/128/256; QT: 16-row query sets (Sq <= 16 QT);
// AL: ALiBi bias; F8: the cache rows are e4m3 bytes with k_scale / v_scale
// (else bf16, scales unused).  st: q and o in bf16 elements, k and v in
// cache elements.  ws: fp32 [B*H, n_chunks, Sq, 2] of (m_c, l_c), then
// [B*H, n_chunks, Sq, D] of acc_c; unused when gridDim.x == 1.
template <int Dp, int QT, bool AL, bool F8>
__global__ __launch_bounds__(DEC_THREADS, (ChunkLds<Dp, QT>::WAVES))
void attn_chunk_partial_kernel(
    const short* __restrict__ q, const char* __restrict__ k,
    const float* __restrict__ k_scale, const char* __restrict__ v,
    const float* __restrict__ v_scale, short* __restrict__ o,
    float* __restrict__ lse_out, float* __restrict__ ws, int H, int Sq,
    int Skv, int D, float scale, const float* __restrict__ alibi,
    const int* __restrict__ kv_lens, AttnStrides st, ScaleStrides sc) {
  using L = ChunkLds<Dp, QT>;
  constexpr int CH = L::CH, QR = L::QR;
  constexpr int RSV = L::RSV, RSQ = L::RSQ, RSP = L::RSP;
  constexpr int KS = Dp / 32;             // k = 32 steps over d
  constexpr int ES = F8 ? 1 : 2;          // bytes per cache element
  constexpr int EPL = 16 / ES;            // cache elements per 16-byte load
  constexpr int KN = Dp / (4 * EPL);      // a lane's loads per K row
  constexpr int GPR = Dp / EPL;           // 16-byte groups per V row
  constexpr int VN = CH * GPR / DEC_THREADS;  // a thread's V loads
  constexpr int QG = QR * (Dp / 8);       // bf16x8 groups of the Q image
  constexpr int QN = (QG + DEC_THREADS - 1) / DEC_THREADS;
  constexpr int DT = Dp / 16, DTW = DT / DEC_WAVES;  // d-tiles, per wave
  static_assert(CH == 32 * DEC_WAVES, "a wave owns 32 keys of the chunk");
  static_assert(CH * GPR % DEC_THREADS == 0 && DT % DEC_WAVES == 0, "");

  const int c = blockIdx.x, n_chunks = gridDim.x;
  const int bh = blockIdx.y;
  const int batch = bh / H, head = bh % H;
  const bool direct = n_chunks == 1;
  const int len = decode_len(kv_lens, batch, Skv);
  const int start = c * CH;
  const int tid = threadIdx.x;
  short* op = o + batch * st.ob + head * st.oh;
  float* lp = lse_out + (int64_t)bh * Sq;

  if (start >= len) {
    // a dead chunk: nothing is loaded and nothing written, unless this
    // workgroup is the whole launch and the slot is empty
    if (direct) {
      for (int i = tid; i < Sq * D; i += DEC_THREADS)
        op[(int64_t)(i / D) * st.os + i % D] = 0;
      if (tid < Sq) lp[tid] = -INFINITY;
    }
    return;
  }
  const int n = min(CH, len - start);  // live rows of this chunk

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int lo = lane & 15, hi = lane >> 4;

  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* v_lds = lds;                      // [CH][RSV]
  short* q_lds = lds + L::V_SHORTS;        // [QR][RSQ], then
  short* p_lds = q_lds;                    // [QR][RSP]
  float* wmax = reinterpret_cast<float*>(lds + L::V_SHORTS + L::QP_SHORTS);
  float* lsum = wmax + DEC_WAVES * QR;     // both [DEC_WAVES][QR]

  const char* kp = k + (batch * st.kb + head * st.kh +
                        (int64_t)start * st.ks) * ES;
  const char* vp = v + (batch * st.vb + head * st.vh +
                        (int64_t)start * st.vs) * ES;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  // Every load below is unconditional and branch-free, so that all of them
  // are in flight together: a dead row reads the chunk's last live row
  // n - 1 and a dead column reads column 0 (both belong to the slot), and
  // the value is then replaced by zeros.

  // ---- K rows into registers: tile kt holds key 32 wave + 16 kt + lo; load
  // i covers columns 4 EPL i + EPL hi .. + EPL ----
  u32x4 kr[2][KN];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int row = 32 * wave + 16 * kt + lo;
#pragma unroll
    for (int i = 0; i < KN; ++i) {
      const int col = 4 * EPL * i + EPL * hi;  // D % 16 == 0: whole or none
      const u32x4 x = *reinterpret_cast<const u32x4*>(
          kp + ((int64_t)min(row, n - 1) * st.ks + (col < D ? col : 0)) * ES);
      kr[kt][i] = (row < n && col < D) ? x : zero;
    }
  }
  // the scales of the 8 keys whose scores this lane will hold
  float ksc[2][4] = {}, vsc[2][4] = {};
  if constexpr (F8) {
    const float* ksp = k_scale + batch * sc.kb + head * sc.kh +
                       (int64_t)start * sc.ks;
    const float* vsp = v_scale + batch * sc.vb + head * sc.vh +
                       (int64_t)start * sc.vs;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 32 * wave + 16 * kt + 4 * hi + r;
        const float ks_ = ksp[(int64_t)min(key, n - 1) * sc.ks];
        const float vs_ = vsp[(int64_t)min(key, n - 1) * sc.vs];
        ksc[kt][r] = key < n ? ks_ : 0.f;
        vsc[kt][r] = key < n ? vs_ : 0.f;
      }
  }

  // ---- V rows into registers, written to LDS after the QK^T MFMAs ----
  u32x4 vr[VN];
#pragma unroll
  for (int it = 0; it < VN; ++it) {
    const int g = tid + it * DEC_THREADS;
    const int row = g / GPR, col = (g % GPR) * EPL;
    const u32x4 x = *reinterpret_cast<const u32x4*>(
        vp + ((int64_t)min(row, n - 1) * st.vs + (col < D ? col : 0)) * ES);
    vr[it] = (row < n && col < D) ? x : zero;
  }

  // ---- Q image: rows past Sq and columns past D are zeros ----
  {
    const short* qp = q + batch * st.qb + head * st.qh;
    u32x4 qr[QN];
#pragma unroll
    for (int it = 0; it < QN; ++it) {
      const int g = tid + it * DEC_THREADS;
      const int row = g / (Dp / 8), col = (g % (Dp / 8)) * 8;
      const u32x4 x = *reinterpret_cast<const u32x4*>(
          qp + (int64_t)min(row, Sq - 1) * st.qs + (col < D ? col : 0));
      qr[it] = (row < Sq && col < D) ? x : zero;
    }
#pragma unroll
    for (int it = 0; it < QN; ++it) {
      const int g = tid + it * DEC_THREADS;
      const int row = g / (Dp / 8), col = (g % (Dp / 8)) * 8;
      if (g < QG) *reinterpret_cast<u32x4*>(q_lds + row * RSQ + col) = qr[it];
    }
  }
  __syncthreads();

  // ---- S^T = K Q^T: s_acc[kt][qt][r] is key 32 wave + 16 kt + 4 hi + r,
  // query 16 qt + lo ----
  f32x4 s_acc[2][QT];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) s_acc[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    // the columns this lane's 8 k-slots of step ks stand for
    const int col = F8 ? (ks >> 1) * 64 + hi * 16 + (ks & 1) * 8
                       : ks * 32 + hi * 8;
    bf16x8 a[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if constexpr (F8) {
        const u32x4 w = kr[kt][ks >> 1];
        a[kt] = __builtin_bit_cast(
            bf16x8, e4m3x8_bf16(w[2 * (ks & 1)], w[2 * (ks & 1) + 1]));
      } else {
        a[kt] = __builtin_bit_cast(bf16x8, kr[kt][ks]);
      }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(
          q_lds + (16 * qt + lo) * RSQ + col);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
        s_acc[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[kt], b, s_acc[kt][qt], 0, 0, 0);
    }
  }
  __builtin_amdgcn_s_setprio(0);

  // ---- V image (e4m3: widened to bf16 here) ----
#pragma unroll
  for (int it = 0; it < VN; ++it) {
    const int g = tid + it * DEC_THREADS;
    const int row = g / GPR, col = (g % GPR) * EPL;
    u32x4* dst = reinterpret_cast<u32x4*>(v_lds + row * RSV + col);
    if constexpr (F8) {
      dst[0] = e4m3x8_bf16(vr[it][0], vr[it][1]);
      dst[1] = e4m3x8_bf16(vr[it][2], vr[it][3]);
    } else {
      dst[0] = vr[it];
    }
  }

  // ---- scores: scale, bias, and the masks where the chunk needs them ----
  const float al_slope = AL ? alibi[head] : 0.f;
  const bool edge = start + CH - 1 > len - Sq;  // causal edge or ragged tail
  float m_c[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = 16 * qt + lo;
    const int pos = len - Sq + qi;  // this query row's position
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 32 * wave + 16 * kt + 4 * hi + r;
        float s = s_acc[kt][qt][r];
        s = F8 ? (s * ksc[kt][r]) * scale : s * scale;
        if (AL) s = fmaf(al_slope, (float)(start + key - pos), s);
        if (edge && (key >= n || start + key > pos)) s = -INFINITY;
        s_acc[kt][qt][r] = s;
        mx = fmaxf(mx, s);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (hi == 0) wmax[wave * QR + qi] = mx;
  }
  __syncthreads();  // row maxima and the V image; Q is dead from here

  // ---- p = exp(s - m_c); fmaxf drops a NaN score, whose p is NaN ----
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = 16 * qt + lo;
    float m = wmax[qi];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) m = fmaxf(m, wmax[w * QR + qi]);
    m_c[qt] = m;
    // a row that sees no key of the chunk has only -inf scores
    const float m_sub = (m == -INFINITY) ? 0.f : m;
    float part = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      float pv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = s_acc[kt][qt][r];
        const float p = __expf(s - m_sub);
        part += p;
        // a masked key's scale is not this row's to see
        pv[r] = F8 ? ((s == -INFINITY) ? 0.f : p * vsc[kt][r]) : p;
      }
      uint2 pk;
      pk.x = pack_bf16(pv[0], pv[1]);
      pk.y = pack_bf16(pv[2], pv[3]);
      *reinterpret_cast<uint2*>(p_lds + qi * RSP + 32 * wave + 16 * kt +
                                4 * hi) = pk;
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (hi == 0) lsum[wave * QR + qi] = part;
  }
  __syncthreads();  // P and the l_c parts

  // ---- O^T = V^T P^T: o_acc[qt][i][r] is d 16 dt + 4 hi + r of query
  // 16 qt + lo, dt = wave + DEC_WAVES i ----
  f32x4 o_acc[QT][DTW];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int i = 0; i < DTW; ++i) o_acc[qt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const short* vrow = v_lds + (4 * hi + (lo >> 2)) * RSV + 4 * (lo & 3);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < CH / 32; ++ks) {
      if (32 * ks >= n) break;  // dead rows only: P = 0 (uniform)
      bf16x8 b[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const short* pr = p_lds + (16 * qt + lo) * RSP + 32 * ks + 4 * hi;
        const bf16x4 b0 = *reinterpret_cast<const bf16x4*>(pr);
        const bf16x4 b1 = *reinterpret_cast<const bf16x4*>(pr + 16);
        b[qt] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < DTW; ++i) {
        const int dt = wave + DEC_WAVES * i;
        if (16 * dt >= D) continue;  // wave-uniform: EXEC stays all ones
        const bf16x4 a0 = lds_read_tr(vrow + (32 * ks) * RSV + 16 * dt);
        const bf16x4 a1 = lds_read_tr(vrow + (32 * ks + 16) * RSV + 16 * dt);
        const bf16x8 a = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6,
                                                 7);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
          o_acc[qt][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, b[qt], o_acc[qt][i], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: the lane holds 4 consecutive d of its query rows ----
  float* ws_acc = ws + (int64_t)gridDim.y * n_chunks * Sq * 2;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = 16 * qt + lo;
    if (qi >= Sq) continue;
    float l = lsum[qi];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) l += lsum[w * QR + qi];
    const float m = m_c[qt];
    const int64_t slot = ((int64_t)bh * n_chunks + c) * Sq + qi;
    if (!direct && wave == 0 && hi == 0) {
      ws[slot * 2] = m;
      ws[slot * 2 + 1] = l;
    }
#pragma unroll
    for (int i = 0; i < DTW; ++i) {
      const int d = 16 * (wave + DEC_WAVES * i) + 4 * hi;
      if (d >= D) continue;  // D % 16 == 0: the lane's 4 d are in or out
      if (direct) {
        short* orow = op + (int64_t)qi * st.os + d;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          attn_decode_finish(o_acc[qt][i][r], l, m, orow + r,
                             (d == 0 && r == 0) ? lp + qi : nullptr);
      } else {
        // 8-byte stores: the acc section starts on an even float
        float2* dst = reinterpret_cast<float2*>(ws_acc + slot * D + d);
        dst[0] = make_float2(o_acc[qt][i][0], o_acc[qt][i][1]);
        dst[1] = make_float2(o_acc[qt][i][2], o_acc[qt][i][3]);
      }
    }
  }
}

// One workgroup per (batch, head, query row); thread t owns head-dim column
// t.  ws as the partial kernel wrote it.
template <int CH>
__global__ __launch_bounds__(DEC_THREADS) void attn_chunk_combine_kernel(
    const float* __restrict__ ws, short* __restrict__ o,
    float* __restrict__ lse_out, int H, int Sq, int Skv, int D, int n_chunks,
    const int* __restrict__ kv_lens, AttnStrides st) {
  const int bh = blockIdx.x, qi = blockIdx.y;
  const int batch = bh / H, head = bh % H;
  const int t = threadIdx.x;
  const int len = decode_len(kv_lens, batch, Skv);
  const int live = (len + CH - 1) / CH;  // chunks that wrote their slots
  const int64_t row0 = (int64_t)bh * n_chunks * Sq + qi;  // chunk 0's slot
  const float* ml = ws + row0 * 2;
  const float* accs = ws + (int64_t)gridDim.x * n_chunks * Sq * 2 + row0 * D;
  float M = -INFINITY;
  for (int c = 0; c < live; ++c) M = fmaxf(M, ml[(int64_t)c * Sq * 2]);
  float L = 0.f, a = 0.f;
  for (int c = 0; c < live; ++c) {
    const float mc = ml[(int64_t)c * Sq * 2];
    const float w = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    L = fmaf(w, ml[(int64_t)c * Sq * 2 + 1], L);
    if (t < D) a = fmaf(w, accs[(int64_t)c * Sq * D + t], a);
  }
  short* orow = o + batch * st.ob + head * st.oh + (int64_t)qi * st.os;
  attn_decode_finish(a, L, M, t < D ? orow + t : nullptr,
                     t == 0 ? lse_out + (int64_t)bh * Sq + qi : nullptr);
}

namespace {

template <int Dp, int QT, bool AL, bool F8>
void chunk_launch(const void* q, const void* k, const float* k_scale,
                  const void* v, const float* v_scale, void* o, float* lse,
                  float* ws, int64_t B, int64_t H, int64_t Sq, int64_t Skv,
                  int64_t D, float scale, const float* alibi,
                  const int* kv_lens, const AttnStrides& st,
                  const ScaleStrides& sc, hipStream_t stream) {
  constexpr int CH = DecodeChunk<Dp>::value;
  const int64_t n_chunks = Skv > 0 ? ceil_div(Skv, CH) : 1;
  dim3 grid((uint32_t)n_chunks, (uint32_t)(B * H));
  attn_chunk_partial_kernel<Dp, QT, AL, F8>
      <<<grid, dim3(DEC_THREADS), ChunkLds<Dp, QT>::BYTES, stream>>>(
          (const short*)q, (const char*)k, k_scale, (const char*)v, v_scale,
          (short*)o, lse, ws, (int)H, (int)Sq, (int)Skv, (int)D, scale,
          alibi, kv_lens, st, sc);
  if (n_chunks > 1)
    attn_chunk_combine_kernel<CH>
        <<<dim3((uint32_t)(B * H), (uint32_t)Sq), dim3(DEC_THREADS), 0,
           stream>>>(ws, (short*)o, lse, (int)H, (int)Sq, (int)Skv, (int)D,
                     (int)n_chunks, kv_lens, st);
}

template <bool F8>
hipError_t chunk_dispatch(const void* q, const void* k, const float* k_scale,
                          const void* v, const float* v_scale, void* o,
                          float* lse, float* ws, int64_t B, int64_t H,
                          int64_t Sq, int64_t Skv, int64_t D, float scale,
                          const float* alibi, const int* kv_lens,
                          const AttnStrides& st, const ScaleStrides& sc,
                          hipStream_t stream) {
  if (D <= 0 || D % 16 != 0 || D > 256 || B * H > 65535 || Sq < 1 || Sq > 64)
    return hipErrorInvalidValue;
#define CHUNK_LAUNCH(DP, QTC, ALB)                                         \
  chunk_launch<DP, QTC, ALB, F8>(q, k, k_scale, v, v_scale, o, lse, ws, B, \
                                 H, Sq, Skv, D, scale, alibi, kv_lens, st, \
                                 sc, stream)
#define CHUNK_QT(DP, ALB)                                                  \
  do {                                                                     \
    if (Sq <= 16) CHUNK_LAUNCH(DP, 1, ALB);                                \
    else if (Sq <= 32) CHUNK_LAUNCH(DP, 2, ALB);                           \
    else CHUNK_LAUNCH(DP, 4, ALB);                                         \
  } while (0)
#define CHUNK_DP(DP)                                                       \
  do {                                                                     \
    if (alibi) CHUNK_QT(DP, true);                                         \
    else CHUNK_QT(DP, false);                                              \
  } while (0)
  if (D <= 64) {
    CHUNK_DP(64);
  } else if (D <= 128) {
    CHUNK_DP(128);
  } else {
    CHUNK_DP(256);
  }
#undef CHUNK_DP
#undef CHUNK_QT
#undef CHUNK_LAUNCH
  return hipGetLastError();
}

}  // namespace

extern "C" {

int64_t attn_chunk_workspace_floats(int64_t B, int64_t H, int64_t Sq,
                                    int64_t Skv, int64_t D) {
  const int64_t n_chunks = ceil_div(Skv, attn_decode_chunk(D));
  return n_chunks <= 1 ? 0 : B * H * n_chunks * Sq * (D + 2);
}

hipError_t launch_attn_chunk(const void* q, const void* k, const void* v,
                             void* o, float* lse, float* ws, int64_t B,
                             int64_t H, int64_t Sq, int64_t Skv, int64_t D,
                             float scale, const float* alibi,
                             const int* kv_lens, const int64_t* strides,
                             hipStream_t stream) {
  return chunk_dispatch<false>(q, k, nullptr, v, nullptr, o, lse, ws, B, H,
                               Sq, Skv, D, scale, alibi, kv_lens,
                               attn_strides(strides), ScaleStrides{}, stream);
}

hipError_t launch_attn_chunk_fp8(const void* q, const void* k8,
                                 const float* k_scale, const void* v8,
                                 const float* v_scale, void* o, float* lse,
                                 float* ws, int64_t B, int64_t H, int64_t Sq,
                                 int64_t Skv, int64_t D, float scale,
                                 const float* alibi, const int* kv_lens,
                                 const int64_t* strides,
                                 hipStream_t stream) {
  const ScaleStrides sc = {strides[12], strides[13], strides[14],
                           strides[15], strides[16], strides[17]};
  return chunk_dispatch<true>(q, k8, k_scale, v8, v_scale, o, lse, ws, B, H,
                              Sq, Skv, D, scale, alibi, kv_lens,
                              attn_strides(strides), sc, stream);
}

}  // extern "C"
