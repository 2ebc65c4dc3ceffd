// Top-k log-prob statistics and top-k / top-p sampling over a row of logits
// (gfx950): the pass over the vocabulary that picks a decode step's next
// token, as two launches with no atomics on global memory and every
// parameter read on the device.
//
// logits [B, V] bf16 or fp32, rows 16-byte aligned.  The working value of
// column j is y_j = float(x_j) * inv_t[b], one fp32 multiply.
//
// Partial kernel, grid (segments, B): a segment is LS_BLOCK * LS_ROUNDS
// 16-byte groups of columns (8192 bf16, 4096 fp32), a constant per dtype, so
// a row's output bits never depend on B, V's other rows or the device.  A
// workgroup reads its segment once, keeps y in registers, and writes the
// segment max m, s = sum exp(y - m) and its min(k, columns) largest (y,
// column) pairs, sorted.
//
// Merge kernel, one workgroup per row: combines the (m, s) in segment order,
// selects the row's top k of the segments' candidates with the same routine,
// writes vals / idx / m / s and, given u, top_k and top_p, draws the token.
//
// Selection (ls_select) is a radix select, not k rounds of argmax: values
// map to order-preserving 32-bit keys; four passes of an 8-bit LDS histogram
// (most significant byte first) find the key T of the k-th largest and the
// number g of keys above it; one ordered compaction (a block scan of packed
// greater / equal counts per round of 16-byte groups) writes the g greater
// items and the first k - g items equal to T, in position order, to LDS; a
// bitonic sort of those <= 128 survivors on (key, ~position) orders them.
// Position order is column order in both kernels (the merge reads segments
// in order, each sorted with equal values by column), so equal values always
// resolve to the lower column, in selection as well as in the output.
#include "common.h"
#include "launchers.h"

#define LS_BLOCK 256
#define LS_ROUNDS 4
#define LS_KMAX 128

struct LsShared {
  uint32_t hist[256];
  uint32_t wsum[LS_BLOCK / 64];
  uint32_t sel[2];
  unsigned long long surv[LS_KMAX];
  float red[LS_BLOCK / 64];
  float p[LS_KMAX];
  int col[LS_KMAX];
};

// fp32 -> key with key(a) > key(b) iff a > b; -0 and +0 share a key.  A NaN
// is an ordinary key at one end: selection never compares floats.
__device__ __forceinline__ uint32_t ls_key(float y) {
  const uint32_t u = (y == 0.0f) ? 0u : __float_as_uint(y);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ls_unkey(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// exclusive prefix of v over the block in thread order and the block total;
// v may pack two 16-bit counters whose totals stay below 65536
__device__ __forceinline__ uint32_t ls_block_scan(uint32_t v, uint32_t* wsum,
                                                  uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < LS_BLOCK / 64; ++w) {
    const uint32_t s = wsum[w];
    if (w < wave) base += s;
    total += s;
  }
  __syncthreads();
  return base + inc - v;
}

__device__ __forceinline__ uint32_t ls_block_min(uint32_t v, uint32_t* wsum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = min(v, (uint32_t)__shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t r = wsum[0];
#pragma unroll
  for (int w = 1; w < LS_BLOCK / 64; ++w) r = min(r, wsum[w]);
  __syncthreads();
  return r;
}

// Item sources of ls_select.  Round r, thread t, element e is position
// (r * LS_BLOCK + t) * kG + e; positions at or past n do not exist.
template <int G>
struct LsRegSrc {  // a segment held in registers
  static constexpr int kG = G;
  const uint32_t (&keys)[LS_ROUNDS * G];
  __device__ __forceinline__ int rounds(int) const { return LS_ROUNDS; }
  __device__ __forceinline__ uint32_t key(int r, int e, int) const {
    return keys[r * G + e];
  }
};

struct LsMemSrc {  // n candidate values in memory
  static constexpr int kG = 1;
  const float* vals;
  __device__ __forceinline__ int rounds(int n) const {
    return (n + LS_BLOCK - 1) / LS_BLOCK;
  }
  __device__ __forceinline__ uint32_t key(int, int, int pos) const {
    return ls_key(vals[pos]);
  }
};

// The k (1 <= k <= min(n, LS_KMAX)) largest of the n items of src, equal
// keys by lower position first: sh.surv[0 .. k) = (key << 32 | ~position),
// descending.  Only items with key >= bound take part; the caller promises
// at least k of them.  Every thread of the block calls it.
template <typename Src>
__device__ __forceinline__ void ls_select(const Src& src, int n, int k,
                                          uint32_t bound, LsShared& sh) {
  constexpr int G = Src::kG;
  const int tid = threadIdx.x;
  const int rounds = src.rounds(n);
  uint32_t prefix = 0, mask = 0, krem = (uint32_t)k;
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
      for (int e = 0; e < G; ++e) {
        const int pos = (r * LS_BLOCK + tid) * G + e;
        if (pos < n) {
          const uint32_t key = src.key(r, e, pos);
          if (key >= bound && (key & mask) == prefix)
            atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
        }
      }
    }
    __syncthreads();
    // thread t looks at bin 255 - t: the scan runs from the largest byte
    const uint32_t c = sh.hist[255 - tid];
    uint32_t total;
    const uint32_t above = ls_block_scan(c, sh.wsum, total);
    if (above < krem && krem <= above + c) {
      sh.sel[0] = 255u - (uint32_t)tid;
      sh.sel[1] = krem - above;
    }
    __syncthreads();
    prefix |= sh.sel[0] << shift;
    mask |= 255u << shift;
    krem = sh.sel[1];
  }
  // prefix is the k-th largest key, krem how many items equal to it are
  // taken (the first in position order), k - krem the number above it
  const uint32_t T = prefix, ngt = (uint32_t)k - krem;
  uint32_t gbase = 0, ebase = 0;
#pragma unroll
  for (int r = 0; r < rounds; ++r) {
    uint32_t cnt = 0;
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int pos = (r * LS_BLOCK + tid) * G + e;
      if (pos < n) {
        const uint32_t key = src.key(r, e, pos);
        cnt += (key > T ? 1u : 0u) + (key == T ? 0x10000u : 0u);
      }
    }
    uint32_t total;
    const uint32_t excl = ls_block_scan(cnt, sh.wsum, total);
    uint32_t gpos = gbase + (excl & 0xffffu), epos = ebase + (excl >> 16);
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int pos = (r * LS_BLOCK + tid) * G + e;
      if (pos < n) {
        const uint32_t key = src.key(r, e, pos);
        const unsigned long long item =
            ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)pos;
        if (key > T) {
          if (gpos < ngt) sh.surv[gpos] = item;  // always true: ngt of them
          ++gpos;
        } else if (key == T) {
          if (epos < krem) sh.surv[ngt + epos] = item;
          ++epos;
        }
      }
    }
    gbase += total & 0xffffu;
    ebase += total >> 16;
  }
  // bitonic sort, descending, of the survivors padded to a power of two
  // with 0, which is below every item (no position is 2^32 - 1)
  int P = 1;
  while (P < k) P <<= 1;
  if (tid >= k && tid < P) sh.surv[tid] = 0ull;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      if (tid < (P >> 1)) {
        const int i = 2 * tid - (tid & (stride - 1)), j = i + stride;
        const unsigned long long a = sh.surv[i], b = sh.surv[j];
        const bool desc = (i & size) == 0;
        if ((a < b) == desc) {
          sh.surv[i] = b;
          sh.surv[j] = a;
        }
      }
    }
  }
  __syncthreads();
}

// G columns from p as fp32: one 16-byte load
__device__ __forceinline__ void ls_load(const short* p, float (&out)[8]) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = bf2f(v[e]);
}

__device__ __forceinline__ void ls_load(const float* p, float (&out)[4]) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = v[e];
}

__device__ __forceinline__ float ls_scalar(const short* p) { return bf2f(*p); }
__device__ __forceinline__ float ls_scalar(const float* p) { return *p; }

// stats [B, nseg, 2] = (m, s); cand_val / cand_col [B, nseg, k], of which
// segment g fills its first min(k, columns of g)
template <typename T, int G>
__global__ __launch_bounds__(LS_BLOCK) void logits_partial_kernel(
    const T* __restrict__ logits, int64_t row_stride,
    const float* __restrict__ inv_t, int V, int k, float* __restrict__ stats,
    float* __restrict__ cand_val, int* __restrict__ cand_col) {
  constexpr int SEG = LS_BLOCK * LS_ROUNDS * G;
  __shared__ LsShared sh;
  const int tid = threadIdx.x;
  const int seg = blockIdx.x, b = blockIdx.y, nseg = gridDim.x;
  const int seg_start = seg * SEG;
  const int cols = min(SEG, V - seg_start);
  const T* row = logits + (int64_t)b * row_stride + seg_start;
  const float it = inv_t[b];

  // one read of the segment; a slot past the row's end holds -inf, which
  // adds nothing to m or s, and never takes part in the selection
  float y[LS_ROUNDS * G];
#pragma unroll
  for (int r = 0; r < LS_ROUNDS; ++r) {
    const int pos0 = (r * LS_BLOCK + tid) * G;
    float x[G];
    if (pos0 + G <= cols) {
      ls_load(row + pos0, x);
    } else {
#pragma unroll
      for (int e = 0; e < G; ++e)
        x[e] = pos0 + e < cols ? ls_scalar(row + pos0 + e) : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < G; ++e) y[r * G + e] = __fmul_rn(x[e], it);
  }

  float tm = -INFINITY;
  int nan = 0;
#pragma unroll
  for (int i = 0; i < LS_ROUNDS * G; ++i) {
    nan |= y[i] != y[i];
    tm = fmaxf(tm, y[i]);
  }
  nan = __syncthreads_or(nan);
  const float m = block_reduce_max(tm, sh.red);
  float ts = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int i = 0; i < LS_ROUNDS * G; ++i) ts += __expf(y[i] - m);
  }
  const float s = block_reduce_sum(ts, sh.red);
  if (tid == 0) {
    float* st = stats + ((int64_t)b * nseg + seg) * 2;
    st[0] = nan ? NAN : m;
    st[1] = nan ? NAN : s;
  }

  // Every thread's largest key is a candidate, so when all LS_BLOCK threads
  // hold a column, at least LS_BLOCK >= k keys reach the smallest of those
  // maxima and nothing below it can be among the k largest: the histograms
  // then see a fraction of the segment.  A thread without a column has
  // maximum 0, which turns the bound off.
  uint32_t keys[LS_ROUNDS * G];
  uint32_t tmax = 0;
#pragma unroll
  for (int r = 0; r < LS_ROUNDS; ++r) {
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int i = r * G + e;
      keys[i] = ls_key(y[i]);
      if ((r * LS_BLOCK + tid) * G + e < cols) tmax = max(tmax, keys[i]);
    }
  }
  const uint32_t bound = ls_block_min(tmax, sh.wsum);
  const int kc = min(k, cols);
  const LsRegSrc<G> src{keys};
  ls_select(src, cols, kc, bound, sh);
  if (tid < kc) {
    const unsigned long long item = sh.surv[tid];
    const int64_t o = ((int64_t)b * nseg + seg) * k + tid;
    cand_val[o] = ls_unkey((uint32_t)(item >> 32));
    cand_col[o] = seg_start + (int)~(uint32_t)item;
  }
}

// u null: no draw.  Else token[b] by the inverse-CDF rule in launchers.h.
__global__ __launch_bounds__(LS_BLOCK) void logits_merge_kernel(
    const float* __restrict__ stats, const float* __restrict__ cand_val,
    const int* __restrict__ cand_col, int nseg, int V, int seg_width, int k,
    int64_t vocab_start, float* __restrict__ vals, int64_t* __restrict__ idx,
    float* __restrict__ m_out, float* __restrict__ s_out,
    const float* __restrict__ u, const int* __restrict__ top_k,
    const float* __restrict__ top_p, int64_t* __restrict__ token) {
  __shared__ LsShared sh;
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* st = stats + (int64_t)b * nseg * 2;
  const float* cv = cand_val + (int64_t)b * nseg * k;
  const int* cc = cand_col + (int64_t)b * nseg * k;
  // every segment but the last is at least LS_KMAX wide and holds k
  // candidates, so the candidates are the first n entries of the row's table
  const int n = (nseg - 1) * k + min(k, V - (nseg - 1) * seg_width);

  if (tid == 0) {
    float M = -INFINITY;
    bool nan = false;
    for (int g = 0; g < nseg; ++g) {
      const float mg = st[2 * g];
      nan |= mg != mg;
      M = fmaxf(M, mg);
    }
    float S = 0.f;
    for (int g = 0; g < nseg; ++g) {
      const float mg = st[2 * g];
      if (mg != -INFINITY) S += st[2 * g + 1] * __expf(mg - M);
    }
    m_out[b] = nan ? NAN : M;
    s_out[b] = nan ? NAN : S;
  }

  const LsMemSrc src{cv};
  ls_select(src, n, k, 0u, sh);
  const float y0 = cv[(int)~(uint32_t)sh.surv[0]];
  if (tid < k) {
    const int pos = (int)~(uint32_t)sh.surv[tid];
    const float yv = cv[pos];
    const int c = cc[pos];
    vals[(int64_t)b * k + tid] = yv;
    idx[(int64_t)b * k + tid] = (int64_t)c + vocab_start;
    sh.p[tid] = __expf(yv - y0);
    sh.col[tid] = c;
  }
  if (u == nullptr) return;
  __syncthreads();
  if (tid == 0) {
    const int tk = top_k[b];
    const int nc = (tk > 0 && tk <= k) ? tk : k;
    int pick = 0;
    if (y0 > -INFINITY) {  // false for -inf and for NaN
      float T = 0.f;
      for (int j = 0; j < nc; ++j) T += sh.p[j];
      const float cut = top_p[b] * T;
      float e = 0.f;
      int kept = 0;
      for (int j = 0; j < nc && (j == 0 || e < cut); ++j) {
        e += sh.p[j];
        kept = j + 1;
      }
      const float want = u[b] * e;  // e is now the kept sum
      pick = kept - 1;
      e = 0.f;
      for (int j = 0; j < kept; ++j) {
        e += sh.p[j];
        if (e > want) {
          pick = j;
          break;
        }
      }
    }
    token[b] = (int64_t)sh.col[pick] + vocab_start;
  }
}

extern "C" {

int logits_topk_segment(int bf16) {
  return LS_BLOCK * LS_ROUNDS * (bf16 ? 8 : 4);
}

hipError_t launch_logits_topk(const void* logits, int bf16,
                              int64_t row_stride, const float* inv_t,
                              int64_t B, int64_t V, int k,
                              int64_t vocab_start, float* stats,
                              float* cand_val, int* cand_col, float* vals,
                              int64_t* idx, float* m, float* s,
                              const float* u, const int* top_k,
                              const float* top_p, int64_t* token,
                              hipStream_t stream) {
  const int seg = logits_topk_segment(bf16);
  const int nseg = (int)ceil_div(V, seg);
  const dim3 grid((uint32_t)nseg, (uint32_t)B);
  if (bf16)
    logits_partial_kernel<short, 8><<<grid, dim3(LS_BLOCK), 0, stream>>>(
        (const short*)logits, row_stride, inv_t, (int)V, k, stats, cand_val,
        cand_col);
  else
    logits_partial_kernel<float, 4><<<grid, dim3(LS_BLOCK), 0, stream>>>(
        (const float*)logits, row_stride, inv_t, (int)V, k, stats, cand_val,
        cand_col);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  logits_merge_kernel<<<dim3((uint32_t)B), dim3(LS_BLOCK), 0, stream>>>(
      stats, cand_val, cand_col, nseg, (int)V, seg, k, vocab_start, vals, idx,
      m, s, u, top_k, top_p, token);
  return hipGetLastError();
}

}  // extern "C"
