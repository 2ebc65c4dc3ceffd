// Tile helpers shared by the attention forward (attention.hip) and backward
// (attention_bwd.hip) kernels for head dims up to 128: the staged-row
// geometry, register-side row fragments, and the three MFMA products the
// kernels are built from.  The k-order permutation of accumulator-derived
// operands and the LDS bank argument are described in the header comment of
// attention_bwd.hip.
#pragma once

#include "common.h"

// ------------------------------------------------------- tile geometry
template <int DK>
struct AttnTile {
  static_assert(DK % 16 == 0 && DK <= 128, "unsupported head-dim tile");
  static constexpr int K32 = DK / 32;          // k = 32 steps over d
  static constexpr bool K16 = (DK % 32) != 0;  // plus 16 more d (half step)
  static constexpr int DT = DK / 16;           // output d-tiles
  static constexpr int RS = K16 ? DK : DK + 16;  // LDS row stride (elements)
  static constexpr int GPR = DK / 8;           // bf16x8 groups per row
  static constexpr int GROUPS = 64 * GPR;      // bf16x8 groups per 64-row tile
  static_assert((RS / 2) % 16 == 8, "row must be an odd multiple of 8 dwords");
};

constexpr float ATTN_LOG2E = 1.4426950408889634f;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16v2 __attribute__((ext_vector_type(2)));

// two f32 -> one dword of two bf16, round-to-nearest-even (the plain cast
// compiles to v_cvt_pk_bf16_f32 and keeps a NaN a NaN)
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16v2));
}

// One row of a [rows][D] operand as the register-side fragment of the
// contraction over d: K32 bf16x8 pieces, plus one for the last 16 d whose
// lane groups 2 and 3 (k-slots 16..31 of that step) hold zeros.
template <int DK>
struct RowFrag {
  bf16x8 w[AttnTile<DK>::K32];
  bf16x8 t;
};

template <int DK>
__device__ __forceinline__ void load_row_frag(RowFrag<DK>& f,
                                              const short* __restrict__ rowp,
                                              int hi, int D) {
  using T = AttnTile<DK>;
#pragma unroll
  for (int ks = 0; ks < T::K32; ++ks) {
    int col = ks * 32 + hi * 8;
    bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    f.w[ks] = z;
    if (col + 8 <= D) f.w[ks] = *reinterpret_cast<const bf16x8*>(rowp + col);
  }
  bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f.t = z8;
  if (T::K16) {
    int col = T::K32 * 32 + hi * 8;
    if (hi < 2 && col + 8 <= D)
      f.t = *reinterpret_cast<const bf16x8*>(rowp + col);
  }
}

// acc[rw] += X[16 rows][d] . F_rw[16 rows][d]^T, contracted over d: A = the
// lane's row of the LDS image (`row` points at its column 0), read once for
// all RW products; B = F_rw in registers.
// Result C[m = X row 4*hi + reg][n = F row lo].
template <int DK, int RW>
__device__ __forceinline__ void rows_x_frags(const short* row, int hi,
                                             const RowFrag<DK> (&b)[RW],
                                             f32x4 (&acc)[RW]) {
  using T = AttnTile<DK>;
  // last 16 d: lane groups 2 and 3 re-read the data of groups 0 and 1,
  // which b[rw].t multiplies by zero
  if (T::K16) {
    bf16x8 a = *reinterpret_cast<const bf16x8*>(row + T::K32 * 32 +
                                                (hi & 1) * 8);
#pragma unroll
    for (int rw = 0; rw < RW; ++rw)
      acc[rw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[rw].t, acc[rw],
                                                        0, 0, 0);
  }
#pragma unroll
  for (int ks = 0; ks < T::K32; ++ks) {
    bf16x8 a = *reinterpret_cast<const bf16x8*>(row + ks * 32 + hi * 8);
#pragma unroll
    for (int rw = 0; rw < RW; ++rw)
      acc[rw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[rw].w[ks],
                                                        acc[rw], 0, 0, 0);
  }
}

// ds_read_b64_tr_b16: each 16-lane group reads a 4-row x 16-column block;
// lane 4q+p of the group addresses row q, columns 4p..4p+3, and lane i
// receives column i of the 4 rows.  Needs EXEC all ones and an 8-byte
// aligned, in-bounds address in every lane.
typedef short __attribute__((address_space(3))) lds_short;
typedef bf16x4 __attribute__((address_space(3))) lds_bf16x4;
__device__ __forceinline__ bf16x4 lds_read_tr(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_bf16x4*)(lds_short*)const_cast<short*>(p));
}

// acc[rw][dt] += A_rw . img[32 rows][16*dt .. 16*dt+15] for every d-tile,
// where A_rw is an accumulator-derived fragment (k order permuted as in the
// header) and `img` points at row 0, column 0 of the 32-row step of a
// row-major image.  Lane (lo, hi) addresses row 4*hi + (lo>>2) (+16 for
// elements 4..7), columns 16*dt + 4*(lo&3); each B fragment is read once
// for all RW products.
template <int DK, int RW>
__device__ __forceinline__ void frags_x_cols(
    const u32x4 (&a)[RW], const short* img, int lo, int hi,
    f32x4 (&acc)[RW][AttnTile<DK>::DT]) {
  using T = AttnTile<DK>;
  const short* p = img + (4 * hi + (lo >> 2)) * T::RS + 4 * (lo & 3);
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) {
    bf16x4 b0 = lds_read_tr(p + dt * 16);
    bf16x4 b1 = lds_read_tr(p + 16 * T::RS + dt * 16);
    bf16x8 b = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int rw = 0; rw < RW; ++rw)
      acc[rw][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, a[rw]), b, acc[rw][dt], 0, 0, 0);
  }
}

// The same product with the operands swapped, so that the result comes out
// transposed: acc[rw][dt] += img[32 rows][16*dt .. 16*dt+15]^T . B_rw, with
// the image columns as A (the same transposed reads as frags_x_cols, each
// feeding RW MFMAs) and the accumulator-derived fragment as B.
// Result C[m = image column 16*dt + 4*hi + reg][n = lo, B_rw's lane index].
template <int DK, int RW>
__device__ __forceinline__ void cols_x_frags(
    const short* img, int lo, int hi, const u32x4 (&b)[RW],
    f32x4 (&acc)[RW][AttnTile<DK>::DT]) {
  using T = AttnTile<DK>;
  const short* p = img + (4 * hi + (lo >> 2)) * T::RS + 4 * (lo & 3);
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) {
    bf16x4 a0 = lds_read_tr(p + dt * 16);
    bf16x4 a1 = lds_read_tr(p + 16 * T::RS + dt * 16);
    bf16x8 a = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int rw = 0; rw < RW; ++rw)
      acc[rw][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a, __builtin_bit_cast(bf16x8, b[rw]), acc[rw][dt], 0, 0, 0);
  }
}
