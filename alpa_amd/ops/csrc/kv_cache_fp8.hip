// kv_cache_append: quantize the new k and v rows of a decoder layer to e4m3
// and write them into the layer's KV cache, in one launch, for gfx950.
//
// Cache format.  k8, v8 [B, H, max_len, D] e4m3 bytes; k_scale, v_scale
// [B, H, max_len] fp32: every row of D values carries its own scale.  A row
// x is stored as
//     scale = amax(|x|) / 448          (fp32 division)
//     byte  = e4m3_rne(x / scale)      (fp32 division, saturating at +-448)
// An all-zero row stores scale = 1 (and the bytes of x / 1).  A row that
// holds a NaN or an Inf stores scale = NaN and the e4m3 NaN code 0x7F in
// every byte, so the whole row dequantizes to NaN; nothing is clamped into
// range silently.  A row's bytes and scale depend on that row alone, so an
// append never touches older rows.
//
// Inputs k, v [B, H, S, D] bf16 are strided views with a contiguous head dim
// (the k and v of the packed qkv projection, k after the rotary transform),
// read in place.  Row (b, h, s) goes to cache position pos_b + s, where
// pos_b is a host int or an int32/int64 device vector [B]; a row whose
// position is negative or >= max_len is skipped entirely, neither loaded nor
// stored.  The kernel reads nothing back to the host and can be captured.
//
// Work split: grid (ceil(B*H*S / rows per workgroup), 2): y = 0 is K, y = 1
// is V.  A row is owned by Dp/8 adjacent lanes (Dp = D padded to 64/128/256,
// the lane map of attention_decode.hip), 16 bytes of bf16 each, so a wave
// holds 8 / 4 / 2 rows and a 256-thread workgroup 32 / 16 / 8.  The row amax
// is an integer max over the |x| bit patterns (NaN > Inf > every finite
// value, so one reduction also finds a non-finite row), reduced by xor
// shuffles inside the lane group.  One lane writes the scale, every live
// lane its 8 bytes with one 8-byte store.  No LDS, no atomics.  The row
// quantize itself is kv_row_quant.h, shared with qkv_cache_write.hip.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage) at every
// Dp: 22 VGPRs, 8 waves per SIMD, no LDS, no scratch.
#include <cstring>

#include "kv_row_quant.h"
#include "launchers.h"

#define KVA_THREADS 256

// (batch, head, seq) strides: sources in bf16 elements, caches in bytes,
// scales in fp32 elements
struct KvAppendStrides {
  int64_t kb, kh, ks;
  int64_t vb, vh, vs;
  int64_t k8b, k8h, k8s;
  int64_t v8b, v8h, v8s;
  int64_t ksb, ksh, kss;
  int64_t vsb, vsh, vss;
};

// pos_kind: 0 host int pos_host, 1 int32 [B] at pos_dev, 2 int64 [B]
template <int Dp>
__global__ __launch_bounds__(KVA_THREADS) void kv_cache_append_kernel(
    const short* __restrict__ k, const short* __restrict__ v,
    unsigned char* __restrict__ k8, float* __restrict__ k_scale,
    unsigned char* __restrict__ v8, float* __restrict__ v_scale, int H, int S,
    int D, int max_len, int64_t n_rows, int64_t pos_host,
    const void* __restrict__ pos_dev, int pos_kind, KvAppendStrides st) {
  constexpr int LPR = Dp / 8;                 // lanes per row
  constexpr int RPB = KVA_THREADS / LPR;      // rows per workgroup
  const bool is_v = blockIdx.y == 1;
  const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int dg = (threadIdx.x % LPR) * 8;     // this lane's 8 columns
  const int s = (int)(r % S);
  const int head = (int)((r / S) % H);
  const int64_t batch = r / ((int64_t)S * H);

  int64_t at = -1;
  if (r < n_rows) {
    const int64_t p0 =
        pos_kind == 0   ? pos_host
        : pos_kind == 1 ? (int64_t) reinterpret_cast<const int*>(pos_dev)[batch]
                        : reinterpret_cast<const int64_t*>(pos_dev)[batch];
    at = p0 + s;
  }
  // the lanes of a skipped row still take part in the shuffles below
  const bool live = r < n_rows && at >= 0 && at < max_len && dg < D;

  bf16x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const short* src = is_v ? v + batch * st.vb + head * st.vh + s * st.vs
                            : k + batch * st.kb + head * st.kh + s * st.ks;
    x = *reinterpret_cast<const bf16x8*>(src + dg);
  }
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(x[j]);
  const unsigned int abits = kv_row_amax_bits<LPR>(f);
  if (!live) return;

  const float scale = kv_row_scale(abits);
  const u32x2 bytes = kv_row_pack(f, abits, scale);
  unsigned char* dst =
      is_v ? v8 + batch * st.v8b + head * st.v8h + at * st.v8s
           : k8 + batch * st.k8b + head * st.k8h + at * st.k8s;
  *reinterpret_cast<u32x2*>(dst + dg) = bytes;
  if (dg == 0) {
    float* sp = is_v ? v_scale + batch * st.vsb + head * st.vsh + at * st.vss
                     : k_scale + batch * st.ksb + head * st.ksh + at * st.kss;
    *sp = scale;
  }
}

extern "C" {

hipError_t launch_kv_cache_append(const void* k, const void* v, void* k8,
                                  float* k_scale, void* v8, float* v_scale,
                                  int64_t B, int64_t H, int64_t S, int64_t D,
                                  int64_t max_len, int64_t pos_host,
                                  const void* pos_dev, int pos_kind,
                                  const int64_t* strides,
                                  hipStream_t stream) {
  if (D < 16 || D % 16 != 0 || D > 256 || max_len > INT32_MAX ||
      H > INT32_MAX || S > INT32_MAX || pos_kind < 0 || pos_kind > 2)
    return hipErrorInvalidValue;
  const int64_t n_rows = B * H * S;
  if (n_rows == 0) return hipSuccess;
  KvAppendStrides st;
  static_assert(sizeof(st) == 18 * sizeof(int64_t), "18 strides");
  memcpy(&st, strides, sizeof(st));
#define KVA_LAUNCH(DP)                                                     \
  do {                                                                     \
    constexpr int RPB = KVA_THREADS / (DP / 8);                            \
    const int64_t blocks = ceil_div(n_rows, RPB);                          \
    if (blocks > INT32_MAX) return hipErrorInvalidValue;                   \
    kv_cache_append_kernel<DP>                                             \
        <<<dim3((uint32_t)blocks, 2), dim3(KVA_THREADS), 0, stream>>>(     \
            (const short*)k, (const short*)v, (unsigned char*)k8, k_scale, \
            (unsigned char*)v8, v_scale, (int)H, (int)S, (int)D,           \
            (int)max_len, n_rows, pos_host, pos_dev, pos_kind, st);        \
  } while (0)
  if (D <= 64) {
    KVA_LAUNCH(64);
  } else if (D <= 128) {
    KVA_LAUNCH(128);
  } else {
    KVA_LAUNCH(256);
  }
#undef KVA_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
