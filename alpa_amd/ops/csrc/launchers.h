// Prototypes of every extern "C" kernel launcher in the library.
//
// Included by each *.hip that defines launchers and by bindings.cpp that
// calls them.  C linkage forbids overloads, so a definition whose parameter
// types or order drift from this header is a compile error instead of a
// clean link that corrupts memory at run time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

extern "C" {

// ---- layernorm.hip ----
hipError_t launch_layer_norm_fwd(const void* x, const void* w, const void* b,
                                 void* y, float* mean, float* rstd, int64_t N,
                                 int64_t H, float eps, hipStream_t stream);
// stripe count P of the backward below: a function of (N, H) alone
int layer_norm_bwd_stripes(int64_t N, int64_t H);
// dx and the dw/db stripe partials [P, H], which launch_colsum_finalize sums;
// one fused kernel for H <= 4096, the dx + dw/db-partial pair for wider rows.
// dh: residual gradient added to dx, or null.  N >= 1.
hipError_t launch_layer_norm_bwd(const void* dy, const void* dh,
                                 const void* x, const void* w,
                                 const float* mean, const float* rstd,
                                 void* dx, float* dw_part, float* db_part,
                                 int64_t N, int64_t H, hipStream_t stream);
hipError_t launch_add_layer_norm_fwd(const void* a, const void* b,
                                     const void* w, const void* bias,
                                     void* h, void* y, float* mean,
                                     float* rstd, int64_t N, int64_t H,
                                     float eps, hipStream_t stream);

// ---- bias_gelu.hip ----
hipError_t launch_bias_gelu_fwd(const void* x, const void* bias, void* y,
                                int64_t N, int64_t F, hipStream_t stream);
// dx and the dbias stripe partials db_part [P, F], in one kernel
hipError_t launch_bias_gelu_bwd(const void* dy, const void* x,
                                const void* bias, void* dx, float* db_part,
                                int64_t N, int64_t F, int P,
                                hipStream_t stream);
hipError_t launch_colsum_partial(const void* t, float* part, int64_t N,
                                 int64_t F, int P, hipStream_t stream);
// out_a[c] = sum over p of part_a[p, c], fixed order, fp32 or (out_bf16)
// bf16 rounded to nearest even; likewise part_b -> out_b in the same launch
// unless part_b is null.  P >= 0, any F >= 1.
hipError_t launch_colsum_finalize(const float* part_a, const float* part_b,
                                  void* out_a, void* out_b, int P, int64_t F,
                                  int out_bf16, hipStream_t stream);

// ---- adamw.hip ----
hipError_t launch_adamw(const void* descs_dev, const void* chunks_dev,
                        int num_chunks, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale,
                        int step, const float* sumsq_or_null, float max_norm,
                        hipStream_t stream);
// sum of squares of every gradient in the table: one fp32 partial per chunk
// into partials [num_chunks], then their fixed-order sum into sumsq [1]
hipError_t launch_multi_tensor_sumsq(const void* descs_dev,
                                     const void* chunks_dev, int num_chunks,
                                     float* partials, float* sumsq,
                                     hipStream_t stream);

// ---- fp8_quant.hip ----
hipError_t launch_fp8_quantize(const void* src, void* q, const float* scale,
                               float* amax, int64_t total, int e5m2,
                               hipStream_t stream);
hipError_t launch_fp8_quantize_dual(const void* src, void* q, void* qt,
                                    const float* scale, float* amax,
                                    int64_t M, int64_t N, int e5m2,
                                    hipStream_t stream);

// ---- fp8_fused.hip ----
// e4m3 only; amax must be zeroed by the caller, as for the quantize above
hipError_t launch_bias_gelu_fp8(const void* x, const void* bias, void* q,
                                void* qt, const float* scale, float* amax,
                                int64_t M, int64_t F, hipStream_t stream);
hipError_t launch_add_layer_norm_fp8(const void* a, const void* b,
                                     const void* w, const void* bias, void* h,
                                     void* q, void* qt, float* mean,
                                     float* rstd, const float* scale,
                                     float* amax, int64_t N, int64_t H,
                                     float eps, hipStream_t stream);

// ---- skinny_gemm.hip ----
hipError_t launch_skinny_gemm(const void* wp, const void* x, float* part,
                              const void* bias_or_null, void* y,
                              const float* wscale_or_null, int64_t M,
                              int64_t MT, int64_t N, int64_t K, int splits,
                              int fp8, hipStream_t stream);

// ---- cross_entropy.hip ----
hipError_t launch_ce_fwd(const void* logits, const int64_t* targets,
                         float* loss, float* lse, int64_t N, int64_t V,
                         hipStream_t stream);
// vocab shard [N, V] holding global columns [vocab_start, vocab_start + V);
// stats: fp32 [3, N] = (row max, sum exp(x - max), owned target logit or 0)
hipError_t launch_ce_partial_fwd(const void* logits, const int64_t* targets,
                                 float* stats, int64_t N, int64_t V,
                                 int64_t vocab_start, hipStream_t stream);
// the full vocab is the shard with vocab_start = 0
hipError_t launch_ce_bwd(const float* dloss, const void* logits,
                         const int64_t* targets, const float* lse,
                         void* dlogits, int64_t N, int64_t V,
                         int64_t vocab_start, hipStream_t stream);

// ---- attention.hip ----
// strides: q(3) k(3) v(3) o(3), each (batch, head, seq) in elements
hipError_t launch_attn_fwd(const void* q, const void* k, const void* v,
                           void* o, float* lse, int64_t B, int64_t H,
                           int64_t S, int64_t Skv, int64_t D, float scale,
                           int causal, const float* alibi,
                           const int* kv_lens, const int64_t* strides,
                           hipStream_t stream);
// strides: q(3) k(3) v(3) do(3) dq(3) dk(3) dv(3) o(3)
hipError_t launch_attn_bwd(const void* q, const void* k, const void* v,
                           const void* o, const void* dout,
                           const float* lse, float* delta_ws, void* dq,
                           void* dk, void* dv, int64_t B, int64_t H,
                           int64_t S, int64_t Skv, int64_t D, float scale,
                           int causal, const float* alibi,
                           const int64_t* strides, hipStream_t stream);

// ---- attention_decode.hip ----
// keys per split-KV chunk at head_dim D: a function of D alone
int attn_decode_chunk(int64_t D);
// fp32 elements of workspace the launch below needs (0 for a single chunk)
int64_t attn_decode_workspace_floats(int64_t B, int64_t H, int64_t Skv,
                                     int64_t D);
// one query row per (batch, head), non-causal over the first kv_lens[b]
// (or Skv) keys; strides as for launch_attn_fwd; q, k, v rows 16-byte
// aligned; o [B,H,1,D] and lse [B*H] are written for every slot
hipError_t launch_attn_decode(const void* q, const void* k, const void* v,
                              void* o, float* lse, float* ws, int64_t B,
                              int64_t H, int64_t Skv, int64_t D, float scale,
                              const float* alibi, const int* kv_lens,
                              const int64_t* strides, hipStream_t stream);

// ---- moe_route.hip ----
// top-2 + in-block ranks (left in slot1/slot2) + per-256-token-block
// histograms and softmax column partials, all [ceil(N/256), E]
hipError_t launch_moe_route(const void* logits, float* w1, float* w2,
                            int* idx1, int* idx2, int* slot1, int* slot2,
                            int* hist1, int* hist2, float* ppart, int64_t N,
                            int64_t E, hipStream_t stream);
// fills src with -1, scans the histograms in place, writes count1 and aux,
// then turns the ranks in slot1/slot2 into slots and fills src
hipError_t launch_moe_slots(const int* idx1, const int* idx2, int* hist1,
                            int* hist2, const float* psum, int* count1,
                            float* aux, int* slot1, int* slot2, int* src,
                            int64_t N, int64_t E, int64_t C,
                            hipStream_t stream);
hipError_t launch_moe_route_bwd(const void* logits, const int* idx1,
                                const int* idx2, const float* w1,
                                const float* w2, const int* count1,
                                const float* dw1, const float* dw2,
                                const float* daux, void* dlogits, int64_t N,
                                int64_t E, hipStream_t stream);
// x [N, H] -> out [S, H]; slot1/w1/w2 all null or all given (scaled rows)
hipError_t launch_moe_dispatch(const void* x, const int* src,
                               const int* slot1_or_null,
                               const float* w1_or_null,
                               const float* w2_or_null, void* out, int64_t S,
                               int64_t N, int64_t H, hipStream_t stream);
// y [S, H] -> out [N, H]; null weights mean 1
hipError_t launch_moe_combine(const void* y, const float* w1_or_null,
                              const float* w2_or_null, const int* slot1,
                              const int* slot2, void* out, int64_t N,
                              int64_t S, int64_t H, hipStream_t stream);
hipError_t launch_moe_combine_dw(const void* dout, const void* y,
                                 const int* slot1, const int* slot2,
                                 float* dw1, float* dw2, int64_t N, int64_t S,
                                 int64_t H, hipStream_t stream);

// ---- mfma_probe.hip ----
hipError_t launch_mfma_probe(const void* a, const void* b, float* d,
                             hipStream_t stream);
hipError_t launch_mfma_probe32(const void* a, const void* b, float* d,
                               hipStream_t stream);

}  // extern "C"
