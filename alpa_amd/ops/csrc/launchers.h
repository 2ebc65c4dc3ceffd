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

// ---- skinny_mfma.hip ----
// 9 <= M <= 64, N % 64 == 0, K % 256 == 0, splits divides K/256 and the
// staged x slice MT * (K/splits + 16) * 2 bytes (MT = 16/32/64, the tier of
// M) is at most SKINNY_MFMA_LDS_MAX.  part_or_null: fp32 [splits, M, N] iff
// splits > 1.  x is [M, K], unpadded.
#define SKINNY_MFMA_LDS_MAX (160 * 1024)
hipError_t launch_skinny_mfma(const void* wp, const void* x,
                              float* part_or_null, const void* bias_or_null,
                              void* y, const float* wscale_or_null,
                              int64_t M, int64_t N, int64_t K, int splits,
                              hipStream_t stream);

// ---- skinny_fp4.hip ----
// MXFP4 weights packed as skinny_fp4.h describes: wq [K/32, N, 16] nibble
// blocks, sq [K/256, N, 8] e8m0 scale bytes, both 16- / 8-byte aligned.
// 1 <= M <= MT, MT = 4 or 8, x [MT, K] with zero rows past M, N % 64 == 0,
// K % 256 == 0, splits divides K/256 and the staged x slice
// (K/splits) * 2 * MT bytes is at most SKINNY_FP4_LDS_MAX.  part: fp32
// [splits, MT, N].
#define SKINNY_FP4_LDS_MAX (64 * 1024)
hipError_t launch_skinny_fp4(const void* wq, const void* sq, const void* x,
                             float* part, const void* bias_or_null, void* y,
                             int64_t M, int64_t MT, int64_t N, int64_t K,
                             int splits, hipStream_t stream);

// ---- skinny_mfma_fp4.hip ----
// the envelope, part_or_null and x of launch_skinny_mfma, over the packed
// MXFP4 weights of launch_skinny_fp4
hipError_t launch_skinny_mfma_fp4(const void* wq, const void* sq,
                                  const void* x, float* part_or_null,
                                  const void* bias_or_null, void* y,
                                  int64_t M, int64_t N, int64_t K, int splits,
                                  hipStream_t stream);

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

// ---- logits_sample.hip ----
// columns per segment of the partial kernel: a function of the dtype alone
int logits_topk_segment(int bf16);
// logits [B, V] bf16 or fp32 with 16-byte-aligned rows row_stride elements
// apart, y = float(x) * inv_t[b]; 1 <= k <= min(V, 128), 1 <= B <= 65535.
// With nseg = ceil(V / segment): workspace stats [B, nseg, 2] fp32 and
// cand_val (fp32) / cand_col (int32) [B, nseg, k].  Writes vals [B, k] (y,
// descending, equal y by lower column), idx [B, k] = column + vocab_start,
// m [B] = max y and s [B] = sum exp(y - m) (0 if m = -inf; both NaN if the
// row holds a NaN).  u null: no draw.  Else u, top_p fp32 [B], top_k int32
// [B] and token [B]: over the first n = (0 < top_k <= k ? top_k : k)
// candidates, p_j = exp(y_j - y_0) summed in ascending j; candidate j is
// kept iff j == 0 or the sum before it is below top_p * total; the token is
// the first kept j whose sum through j exceeds u * (kept sum), else the last
// kept; candidate 0 if y_0 is -inf or NaN
hipError_t launch_logits_topk(const void* logits, int bf16,
                              int64_t row_stride, const float* inv_t,
                              int64_t B, int64_t V, int k,
                              int64_t vocab_start, float* stats,
                              float* cand_val, int* cand_col, float* vals,
                              int64_t* idx, float* m, float* s,
                              const float* u, const int* top_k,
                              const float* top_p, int64_t* token,
                              hipStream_t stream);

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

// ---- attention_decode_fp8.hip ----
// launch_attn_decode over an e4m3 cache: k8, v8 [B,H,Skv,D] bytes with 16-
// byte-aligned rows, k_scale, v_scale [B,H,Skv] fp32, one scale per row.
// strides: q(3) k8(3) v8(3) o(3) k_scale(3) v_scale(3), each (batch, head,
// seq) in elements; chunking and workspace as for launch_attn_decode
hipError_t launch_attn_decode_fp8(const void* q, const void* k8,
                                  const float* k_scale, const void* v8,
                                  const float* v_scale, void* o, float* lse,
                                  float* ws, int64_t B, int64_t H,
                                  int64_t Skv, int64_t D, float scale,
                                  const float* alibi, const int* kv_lens,
                                  const int64_t* strides, hipStream_t stream);

// ---- attention_chunk.hip ----
// 1 <= Sq <= 64 query rows per (batch, head) over a cache that already holds
// them: row i sits at position len_b - Sq + i and sees keys j <= that
// (len_b = kv_lens[b] clamped to [0, Skv], or Skv).  Operands, strides and
// chunking as for launch_attn_decode / launch_attn_decode_fp8; o [B,H,Sq,D]
// and lse [B*H*Sq] are written for every row
int64_t attn_chunk_workspace_floats(int64_t B, int64_t H, int64_t Sq,
                                    int64_t Skv, int64_t D);
hipError_t launch_attn_chunk(const void* q, const void* k, const void* v,
                             void* o, float* lse, float* ws, int64_t B,
                             int64_t H, int64_t Sq, int64_t Skv, int64_t D,
                             float scale, const float* alibi,
                             const int* kv_lens, const int64_t* strides,
                             hipStream_t stream);
hipError_t launch_attn_chunk_fp8(const void* q, const void* k8,
                                 const float* k_scale, const void* v8,
                                 const float* v_scale, void* o, float* lse,
                                 float* ws, int64_t B, int64_t H, int64_t Sq,
                                 int64_t Skv, int64_t D, float scale,
                                 const float* alibi, const int* kv_lens,
                                 const int64_t* strides, hipStream_t stream);

// ---- kv_cache_fp8.hip ----
// quantize k, v [B,H,S,D] bf16 (16-byte-aligned rows) per row to e4m3 and
// write row (b, h, s) at cache position pos_b + s of k8/v8 [B,H,max_len,D]
// (8-byte-aligned rows) and k_scale/v_scale [B,H,max_len]; positions outside
// [0, max_len) are skipped.  pos_kind 0: pos_b = pos_host; 1 / 2: pos_dev is
// int32 / int64 [B].  strides: k(3) v(3) k8(3) v8(3) k_scale(3) v_scale(3)
hipError_t launch_kv_cache_append(const void* k, const void* v, void* k8,
                                  float* k_scale, void* v8, float* v_scale,
                                  int64_t B, int64_t H, int64_t S, int64_t D,
                                  int64_t max_len, int64_t pos_host,
                                  const void* pos_dev, int pos_kind,
                                  const int64_t* strides, hipStream_t stream);

// ---- qkv_cache_write.hip ----
// split the packed qkv [B,S,H,3,D] bf16 (16-byte-aligned rows), rotate q and
// k (table_kind 0: no rotary; 1 / 2: sin_t, cos_t [T, rotary_dim/2] fp32 /
// bf16), write q_out and (unless null) k_new [B,H,S,D] contiguous, and write
// k and v at row pos_b + s of the cache: cache_fp8 0, bf16 [B,H,L,D] with
// 16-byte-aligned rows (scales null); 1, the e4m3 cache of kv_cache_fp8.hip.
// A row whose position is outside [0, L), or outside the tables, is written
// as zeros to q_out / k_new and not at all to the cache.  pos_kind as in
// launch_kv_cache_append.  strides: qkv (batch, seq, head), cache_k(3),
// cache_v(3), k_scale(3), v_scale(3)
hipError_t launch_qkv_cache_write(
    const void* qkv, void* q_out, void* k_new, void* cache_k, void* cache_v,
    float* k_scale, float* v_scale, int cache_fp8, const void* sin_t,
    const void* cos_t, int table_kind, int64_t rotary_dim, int64_t T,
    int64_t B, int64_t S, int64_t H, int64_t D, int64_t L, int64_t pos_host,
    const void* pos_dev, int pos_kind, const int64_t* strides,
    hipStream_t stream);

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
