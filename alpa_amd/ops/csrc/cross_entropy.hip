// Fused softmax-cross-entropy over the vocab dim (gfx950).
//
// logits [N, V] bf16 (V = 51200 for the GPT ladder), targets [N] int64.
// Forward: one block per row, single online max+sumexp pass (never
// materializes a softmax tensor).  Backward: dlogits = (softmax - onehot)
// * dloss recomputed from (logits, lse).  With the vocab sharded over
// tensor-parallel ranks the same row pass gives each shard's combinable
// (max, sum-exp, target logit), and the backward runs per shard off the
// global lse.
#include "common.h"
#include "launchers.h"

#define CE_BLOCK 256

// One row's online max + sum(exp(x - max)) pass, shared by the full-vocab
// forward and the vocab-shard partial forward.  Every thread of the block
// calls it (it holds block barriers); all return the row max `gm` and
// `gs` = sum(exp(x - gm)), reduced in a fixed order.  A row with nothing
// finite gives gm = -inf and gs = 0, never NaN.  `red`: CE_BLOCK / 64
// floats of LDS.
__device__ __forceinline__ void ce_row_max_sumexp(const short* __restrict__ lr,
                                                  int V, float* red,
                                                  float& gm, float& gs) {
  // online max + sum(exp(x - m))
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x * 8; i < V; i += CE_BLOCK * 8) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(lr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      if (f > m) {
        s *= __expf(m - f);
        m = f;
      }
      // a -inf logit (masked vocab slot) adds nothing; while m is still
      // -inf, f - m would be inf - inf = NaN
      if (f != -INFINITY) s += __expf(f - m);
    }
  }
  // combine across block: need global max first.  A thread that saw
  // nothing finite (or no element at all) still has m = -inf and s = 0.
  gm = block_reduce_max(m, red);
  s = (m == -INFINITY) ? 0.f : s * __expf(m - gm);
  gs = block_reduce_sum(s, red);
}

// Column of this row's target inside a shard that starts at global vocab
// id `vocab_start` and is V wide, or -1 when the shard does not own it
// (negative ids and ids past the vocab included).  Callers index the row
// only with a result >= 0.
__device__ __forceinline__ int ce_local_target(int64_t target,
                                               int64_t vocab_start, int V) {
  if (target < vocab_start || target - vocab_start >= (int64_t)V) return -1;
  return (int)(target - vocab_start);
}

__global__ void ce_fwd_kernel(const short* __restrict__ logits,
                              const int64_t* __restrict__ targets,
                              float* __restrict__ loss,
                              float* __restrict__ lse_out, int V) {
  const int row = blockIdx.x;
  const short* lr = logits + (int64_t)row * V;
  __shared__ float red[CE_BLOCK / 64];

  float gm, gs;
  ce_row_max_sumexp(lr, V, red, gm, gs);
  float lse = gm + __logf(gs);
  if (threadIdx.x == 0) {
    int64_t t = targets[row];
    loss[row] = lse - bf2f(lr[t]);
    lse_out[row] = lse;
  }
}

// Vocab-shard forward: logits [N, V] is one rank's slice of the vocab,
// columns [vocab_start, vocab_start + V) of the global one.  Writes the
// combinable row statistics stats [3, N]: the local max m, s = sum(exp(x -
// m)) (0 when m = -inf) and t = the target logit if this shard owns the
// target, else 0.
__global__ void ce_partial_fwd_kernel(const short* __restrict__ logits,
                                      const int64_t* __restrict__ targets,
                                      float* __restrict__ stats, int N, int V,
                                      int64_t vocab_start) {
  const int row = blockIdx.x;
  const short* lr = logits + (int64_t)row * V;
  __shared__ float red[CE_BLOCK / 64];

  float gm, gs;
  ce_row_max_sumexp(lr, V, red, gm, gs);
  if (threadIdx.x == 0) {
    const int t = ce_local_target(targets[row], vocab_start, V);
    stats[row] = gm;
    stats[(int64_t)N + row] = gs;
    stats[2 * (int64_t)N + row] = t >= 0 ? bf2f(lr[t]) : 0.f;
  }
}

// dlogits = (exp(x - lse) - onehot) * dloss over a vocab shard (the whole
// vocab when vocab_start = 0 and V is the full width); lse is the row's
// global log-sum-exp.  A shard that does not own the target subtracts no
// one-hot.
__global__ void ce_bwd_kernel(const float* __restrict__ dloss,
                              const short* __restrict__ logits,
                              const int64_t* __restrict__ targets,
                              const float* __restrict__ lse,
                              short* __restrict__ dlogits, int V,
                              int64_t vocab_start) {
  const int row = blockIdx.x;
  const short* lr = logits + (int64_t)row * V;
  short* dr = dlogits + (int64_t)row * V;
  const float l = lse[row];
  const float dl = dloss[row];
  const int t = ce_local_target(targets[row], vocab_start, V);
  for (int i = threadIdx.x * 8; i < V; i += CE_BLOCK * 8) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(lr + i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float p = __expf(bf2f(v[j]) - l);
      if (i + j == t) p -= 1.0f;
      o[j] = f2bf(p * dl);
    }
    *reinterpret_cast<bf16x8*>(dr + i) = o;
  }
}

extern "C" {

hipError_t launch_ce_fwd(const void* logits, const int64_t* targets,
                         float* loss, float* lse, int64_t N, int64_t V,
                         hipStream_t stream) {
  ce_fwd_kernel<<<dim3((uint32_t)N), dim3(CE_BLOCK), 0, stream>>>(
      (const short*)logits, targets, loss, lse, (int)V);
  return hipGetLastError();
}

hipError_t launch_ce_partial_fwd(const void* logits, const int64_t* targets,
                                 float* stats, int64_t N, int64_t V,
                                 int64_t vocab_start, hipStream_t stream) {
  ce_partial_fwd_kernel<<<dim3((uint32_t)N), dim3(CE_BLOCK), 0, stream>>>(
      (const short*)logits, targets, stats, (int)N, (int)V, vocab_start);
  return hipGetLastError();
}

hipError_t launch_ce_bwd(const float* dloss, const void* logits,
                         const int64_t* targets, const float* lse,
                         void* dlogits, int64_t N, int64_t V,
                         int64_t vocab_start, hipStream_t stream) {
  ce_bwd_kernel<<<dim3((uint32_t)N), dim3(CE_BLOCK), 0, stream>>>(
      dloss, (const short*)logits, targets, lse, (short*)dlogits, (int)V,
      vocab_start);
  return hipGetLastError();
}

}  // extern "C"
