// qkv_cache_write: everything between the packed qkv projection and the
// attention kernel of a cached decoder step, in one launch, for gfx950.
//
// Input qkv [B, S, H, 3, D] bf16, a strided view of the projection output
// (head dim contiguous, the q, k and v rows of a (b, s, head) triple D apart,
// every row 16-byte aligned), read in place.  Row (b, head, s) sits at
// position p = pos_b + s, pos_b a host int or an int32/int64 device vector
// [B] that only the device reads, so the launch can be captured.
//   q      [B, H, S, D] bf16 contiguous: q, rotated
//   k_new  [B, H, S, D] bf16 contiguous: k, rotated (optional)
//   cache  row p of slot b, head: k rotated, v as it is.  bf16 cache: views
//          [B, H, L, D] with 16-byte-aligned rows.  e4m3 cache: the bytes and
//          per-row fp32 scales of kv_cache_fp8.hip, 8-byte-aligned rows,
//          quantized from the bf16-ROUNDED rotated row by kv_row_quant.h, so
//          they are the bytes kv_cache_append makes of k_new and v.
//
// Rotary (GPT-J interleaved pairs on the first rotary_dim columns): for the
// pair (x0, x1) at columns (2i, 2i+1) and s = sin[p, i], c = cos[p, i],
// tables [T, rotary_dim/2] fp32 or bf16 converted to fp32,
//     y0 = bf16_rne(x0*c - x1*s)      y1 = bf16_rne(x0*s + x1*c)
// with every multiply, add and subtract rounded on its own in fp32 (contract
// is off in qcw_rotate: it compiles to 16 v_mul_f32, 8 v_sub_f32 and 8
// v_add_f32 per lane; the fused forms left in the ISA belong to the IEEE
// divisions of the row quantize and the index divisions).  Columns at or past
// rotary_dim and all of v are copied bit for bit.  A NaN result is stored as
// 0x7FC0.
//
// A row is valid if 0 <= p < L and, with rotary, p < T.  For an invalid row
// nothing is loaded (qkv and tables alike), nothing is written to either
// cache, scales included, and the q row (and k_new row) is written as zeros.
//
// Work split.  A task is one (b, s, head) triple, in that order, so the 3*D
// contiguous elements of consecutive tasks are consecutive in memory.  It is
// owned by Dp/8 adjacent lanes (Dp = D padded to 64/128/256, the lane map of
// kv_cache_fp8.hip and attention_decode.hip), 16 bytes of each of the three
// rows per lane.  A lane's 8 columns are 4 whole pairs and rotary_dim % 8 ==
// 0, so a lane is wholly rotated or wholly copied and needs no other lane's
// data.  The lane group reads its slot's position, then issues its three row
// loads and one vector load per table (4 sin, 4 cos: 16 bytes fp32, 8 bytes
// bf16; the same registers serve q and k) before any math.  Stores: 16 bytes
// for q, k_new and each bf16 cache row; 8 bytes for each e4m3 cache row, and
// the lane with column 0 writes the two scales.  Dead lanes (column >= D),
// skipped rows and tasks past the end stay for the amax shuffles of the e4m3
// path and leave after them.  No LDS, no atomics.  Cache kind and table
// dtype / rotary off are template parameters; k_new given or not is a
// launch-uniform branch.
//
// Workgroup size: a decode launch has only B*H tasks (OPT-13B batch 1: 40
// tasks, 10 waves), so up to QCW_SMALL_WAVES waves the launcher uses one-wave
// workgroups, which the dispatcher spreads over as many CUs; larger launches
// (prefill: B*S*H tasks) use 256 threads.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage), all Dp:
//   bf16 cache: no rotary 28 VGPRs, fp32 tables 45, bf16 tables 43
//   e4m3 cache: no rotary 31 VGPRs (32 at Dp 256), fp32 tables 44, bf16
//   tables 42
// 8 waves per SIMD, no LDS, no scratch in every instantiation.
#include <cstring>

#include "kv_row_quant.h"
#include "launchers.h"

#define QCW_THREADS 256
#define QCW_SMALL_WAVES 1024

// qkv (batch, seq, head) strides in bf16 elements; cache (batch, head, row)
// strides in elements of the cache (bf16, or bytes for e4m3); scale strides
// in fp32 elements (unused with a bf16 cache)
struct QkvWriteStrides {
  int64_t xb, xs, xh;
  int64_t kb, kh, kl;
  int64_t vb, vh, vl;
  int64_t ksb, ksh, ksl;
  int64_t vsb, vsh, vsl;
};

enum { QCW_ROT_NONE = 0, QCW_ROT_F32 = 1, QCW_ROT_BF16 = 2 };

// bf16 round-to-nearest-even with torch's NaN (0x7FC0)
__device__ __forceinline__ short qcw_round(float y) {
  return y != y ? (short)0x7fc0 : f2bf(y);
}

// the 4 interleaved pairs of one lane, each operation rounded on its own
__device__ __forceinline__ bf16x8 qcw_rotate(bf16x8 x, const float (&sn)[4],
                                             const float (&cs)[4]) {
#pragma clang fp contract(off)
  bf16x8 y;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = bf2f(x[2 * i]), x1 = bf2f(x[2 * i + 1]);
    const float a = x0 * cs[i];
    const float b = x1 * sn[i];
    const float c = x0 * sn[i];
    const float d = x1 * cs[i];
    y[2 * i] = qcw_round(a - b);
    y[2 * i + 1] = qcw_round(c + d);
  }
  return y;
}

// pos_kind: 0 host int pos_host, 1 int32 [B] at pos_dev, 2 int64 [B]
template <int Dp, bool FP8, int ROT>
__global__ __launch_bounds__(QCW_THREADS) void qkv_cache_write_kernel(
    const short* __restrict__ qkv, short* __restrict__ q_out,
    short* __restrict__ k_new, void* __restrict__ cache_k,
    void* __restrict__ cache_v, float* __restrict__ k_scale,
    float* __restrict__ v_scale, const void* __restrict__ sin_t,
    const void* __restrict__ cos_t, int rotary_dim, int64_t T, int H, int S,
    int D, int64_t L, unsigned int n_tasks, int64_t pos_host,
    const void* __restrict__ pos_dev, int pos_kind, QkvWriteStrides st) {
  constexpr int LPR = Dp / 8;                       // lanes per task
  const int tpb = blockDim.x / LPR;                 // tasks per workgroup
  // n_tasks < 2^31 (the launcher checks), so task indices fit 32 bits
  const unsigned int r = blockIdx.x * tpb + threadIdx.x / LPR;
  const int dg = (threadIdx.x % LPR) * 8;           // this lane's 8 columns
  const unsigned int bs = r / (unsigned int)H;
  const int head = (int)(r - bs * (unsigned int)H);
  const int64_t batch = bs / (unsigned int)S;
  const int s = (int)(bs - (unsigned int)batch * (unsigned int)S);
  const bool mine = r < n_tasks && dg < D;          // a lane with a q to write

  int64_t p = -1;
  if (r < n_tasks) {
    const int64_t p0 =
        pos_kind == 0   ? pos_host
        : pos_kind == 1 ? (int64_t) reinterpret_cast<const int*>(pos_dev)[batch]
                        : reinterpret_cast<const int64_t*>(pos_dev)[batch];
    p = p0 + s;
  }
  const bool valid = p >= 0 && p < L && (ROT == QCW_ROT_NONE || p < T);
  const bool live = mine && valid;
  const bool rot = ROT != QCW_ROT_NONE && live && dg < rotary_dim;

  // every load of the task, before any math
  bf16x8 xq = {0, 0, 0, 0, 0, 0, 0, 0}, xk = xq, xv = xq;
  if (live) {
    const short* src =
        qkv + batch * st.xb + s * st.xs + head * st.xh + dg;
    xq = *reinterpret_cast<const bf16x8*>(src);
    xk = *reinterpret_cast<const bf16x8*>(src + D);
    xv = *reinterpret_cast<const bf16x8*>(src + 2 * D);
  }
  float sn[4] = {0.f, 0.f, 0.f, 0.f}, cs[4] = {1.f, 1.f, 1.f, 1.f};
  if (rot) {
    const int64_t at = p * (rotary_dim / 2) + dg / 2;
    if (ROT == QCW_ROT_F32) {
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(
          reinterpret_cast<const float*>(sin_t) + at);
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(
          reinterpret_cast<const float*>(cos_t) + at);
#pragma unroll
      for (int i = 0; i < 4; ++i) sn[i] = s4[i], cs[i] = c4[i];
    } else {
      const bf16x4 s4 = *reinterpret_cast<const bf16x4*>(
          reinterpret_cast<const short*>(sin_t) + at);
      const bf16x4 c4 = *reinterpret_cast<const bf16x4*>(
          reinterpret_cast<const short*>(cos_t) + at);
#pragma unroll
      for (int i = 0; i < 4; ++i) sn[i] = bf2f(s4[i]), cs[i] = bf2f(c4[i]);
    }
  }
  if (rot) {
    xq = qcw_rotate(xq, sn, cs);
    xk = qcw_rotate(xk, sn, cs);
  }

  if (mine) {                     // an invalid row is written as zeros
    const int64_t o = ((batch * H + head) * S + s) * D + dg;
    *reinterpret_cast<bf16x8*>(q_out + o) = xq;
    if (k_new != nullptr) *reinterpret_cast<bf16x8*>(k_new + o) = xk;
  }

  if (!FP8) {
    if (!live) return;
    short* ck = reinterpret_cast<short*>(cache_k);
    short* cv = reinterpret_cast<short*>(cache_v);
    *reinterpret_cast<bf16x8*>(ck + batch * st.kb + head * st.kh + p * st.kl +
                               dg) = xk;
    *reinterpret_cast<bf16x8*>(cv + batch * st.vb + head * st.vh + p * st.vl +
                               dg) = xv;
  } else {
    float fk[8], fv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) fk[j] = bf2f(xk[j]), fv[j] = bf2f(xv[j]);
    // the lanes that hold zeros still take part in the shuffles
    const unsigned int ak = kv_row_amax_bits<LPR>(fk);
    const unsigned int av = kv_row_amax_bits<LPR>(fv);
    if (!live) return;
    const float sk = kv_row_scale(ak), sv = kv_row_scale(av);
    unsigned char* ck = reinterpret_cast<unsigned char*>(cache_k);
    unsigned char* cv = reinterpret_cast<unsigned char*>(cache_v);
    *reinterpret_cast<u32x2*>(ck + batch * st.kb + head * st.kh + p * st.kl +
                              dg) = kv_row_pack(fk, ak, sk);
    *reinterpret_cast<u32x2*>(cv + batch * st.vb + head * st.vh + p * st.vl +
                              dg) = kv_row_pack(fv, av, sv);
    if (dg == 0) {
      k_scale[batch * st.ksb + head * st.ksh + p * st.ksl] = sk;
      v_scale[batch * st.vsb + head * st.vsh + p * st.vsl] = sv;
    }
  }
}

namespace {

struct QcwArgs {
  const short* qkv;
  short *q_out, *k_new;
  void *cache_k, *cache_v;
  float *k_scale, *v_scale;
  const void *sin_t, *cos_t;
  int rotary_dim;
  int64_t T;
  int H, S, D;
  int64_t L, n_tasks, pos_host;
  const void* pos_dev;
  int pos_kind;
  QkvWriteStrides st;
};

template <int Dp, bool FP8, int ROT>
hipError_t qcw_launch(const QcwArgs& a, hipStream_t stream) {
  constexpr int LPR = Dp / 8;
  const int64_t waves = ceil_div(a.n_tasks * LPR, 64);
  const int threads = waves <= QCW_SMALL_WAVES ? 64 : QCW_THREADS;
  const int64_t blocks = ceil_div(a.n_tasks, threads / LPR);
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  qkv_cache_write_kernel<Dp, FP8, ROT>
      <<<dim3((uint32_t)blocks), dim3(threads), 0, stream>>>(
          a.qkv, a.q_out, a.k_new, a.cache_k, a.cache_v, a.k_scale, a.v_scale,
          a.sin_t, a.cos_t, a.rotary_dim, a.T, a.H, a.S, a.D, a.L,
          (unsigned int)a.n_tasks,
          a.pos_host, a.pos_dev, a.pos_kind, a.st);
  return hipGetLastError();
}

template <bool FP8, int ROT>
hipError_t qcw_by_dim(const QcwArgs& a, hipStream_t stream) {
  if (a.D <= 64) return qcw_launch<64, FP8, ROT>(a, stream);
  if (a.D <= 128) return qcw_launch<128, FP8, ROT>(a, stream);
  return qcw_launch<256, FP8, ROT>(a, stream);
}

template <bool FP8>
hipError_t qcw_by_rot(int rot, const QcwArgs& a, hipStream_t stream) {
  if (rot == QCW_ROT_NONE) return qcw_by_dim<FP8, QCW_ROT_NONE>(a, stream);
  if (rot == QCW_ROT_F32) return qcw_by_dim<FP8, QCW_ROT_F32>(a, stream);
  return qcw_by_dim<FP8, QCW_ROT_BF16>(a, stream);
}

}  // namespace

extern "C" {

hipError_t launch_qkv_cache_write(
    const void* qkv, void* q_out, void* k_new, void* cache_k, void* cache_v,
    float* k_scale, float* v_scale, int cache_fp8, const void* sin_t,
    const void* cos_t, int table_kind, int64_t rotary_dim, int64_t T,
    int64_t B, int64_t S, int64_t H, int64_t D, int64_t L, int64_t pos_host,
    const void* pos_dev, int pos_kind, const int64_t* strides,
    hipStream_t stream) {
  if (D < 16 || D % 16 != 0 || D > 256 || H > INT32_MAX || S > INT32_MAX ||
      pos_kind < 0 || pos_kind > 2 || table_kind < QCW_ROT_NONE ||
      table_kind > QCW_ROT_BF16)
    return hipErrorInvalidValue;
  if (table_kind != QCW_ROT_NONE &&
      (rotary_dim <= 0 || rotary_dim % 8 != 0 || rotary_dim > D ||
       sin_t == nullptr || cos_t == nullptr || T < 0))
    return hipErrorInvalidValue;
  if (cache_fp8 && (k_scale == nullptr || v_scale == nullptr))
    return hipErrorInvalidValue;
  QcwArgs a;
  a.qkv = (const short*)qkv;
  a.q_out = (short*)q_out;
  a.k_new = (short*)k_new;
  a.cache_k = cache_k;
  a.cache_v = cache_v;
  a.k_scale = k_scale;
  a.v_scale = v_scale;
  a.sin_t = sin_t;
  a.cos_t = cos_t;
  a.rotary_dim = (int)rotary_dim;
  a.T = T;
  a.H = (int)H;
  a.S = (int)S;
  a.D = (int)D;
  a.L = L;
  a.n_tasks = B * S * H;
  a.pos_host = pos_host;
  a.pos_dev = pos_dev;
  a.pos_kind = pos_kind;
  static_assert(sizeof(a.st) == 15 * sizeof(int64_t), "15 strides");
  memcpy(&a.st, strides, sizeof(a.st));
  if (a.n_tasks == 0) return hipSuccess;
  if (a.n_tasks > INT32_MAX) return hipErrorInvalidValue;
  return cache_fp8 ? qcw_by_rot<true>(table_kind, a, stream)
                   : qcw_by_rot<false>(table_kind, a, stream);
}

}  // extern "C"
