// Python bindings for the gfx950 kernel library (native HIP — no hipify).
//
// Tensor checking + allocation happens here; kernels live in *.hip files
// exposing extern "C" launchers over raw pointers + hipStream_t.
#include <torch/extension.h>

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <vector>
#include <algorithm>
#include <array>
#include <utility>

#include "launchers.h"

#define HIP_OK(expr)                                                       \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));   \
  } while (0)

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---------------------------- operand checks -----------------------------
// Every entry below examines every tensor it hands to a launcher with one of
// these, before it allocates or launches.  `first` is the entry's first
// tensor operand (itself, for that operand): all operands share its device.

const char* dtype_name(at::ScalarType dtype) {
  switch (dtype) {
    case at::kBFloat16: return "bf16";
    case at::kFloat: return "fp32";
    case at::kInt: return "int32";
    case at::kLong: return "int64";
    default: return c10::toString(dtype);
  }
}

// on the GPU, on the device of the first operand
void check_device(const at::Tensor& t, const char* name,
                  const at::Tensor& first) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.device() == first.device(), name, " is on ", t.device(),
              " but the first operand is on ", first.device());
}

// a device operand of one scalar type
void check_typed(const at::Tensor& t, const char* name, at::ScalarType dtype,
                 const at::Tensor& first) {
  check_device(t, name, first);
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype_name(dtype));
}

// a vector or statistics tensor: contiguous, n elements of one type (bf16
// per-feature vectors read with 16-byte loads, fp32 row statistics and
// scalars, int32/int64 index vectors)
void check_vec(const at::Tensor& t, const char* name, at::ScalarType dtype,
               int64_t n, const at::Tensor& first) {
  check_typed(t, name, dtype, first);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " elements, got ",
              t.numel());
}

// row-major bf16 rows [.., W] with W a positive multiple of m (8 for the
// kernels that read rows with 16-byte loads); returns (N, W).  The only
// place that divides numel() by a width: W > 0 is checked just above it.
std::pair<int64_t, int64_t> check_rows(const at::Tensor& t, const char* name,
                                       int64_t m, const at::Tensor& first) {
  check_typed(t, name, at::kBFloat16, first);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() >= 1, name, " must have a feature dimension");
  const int64_t W = t.size(-1);
  TORCH_CHECK(W > 0 && W % m == 0, name,
              ": the last dimension must be a positive multiple of ", m,
              ", got ", W);
  return {t.numel() / W, W};
}

// a second bf16 operand that the kernel indexes exactly like `ref`
void check_like(const at::Tensor& t, const char* name, const at::Tensor& ref,
                const char* ref_name) {
  check_typed(t, name, at::kBFloat16, ref);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.sizes() == ref.sizes(), name, " must have the shape of ",
              ref_name);
}

// a logical [B, H, S, D] bf16 view with arbitrary B/H/S strides and a
// contiguous D; a negative expected size accepts any
void check_bhsd(const at::Tensor& t, const char* name, int64_t B, int64_t H,
                int64_t S, int64_t D, const at::Tensor& first) {
  check_typed(t, name, at::kBFloat16, first);
  TORCH_CHECK(t.dim() == 4, name, " must be 4-D [B,H,S,D]");
  TORCH_CHECK(t.stride(3) == 1, name, " head-dim must be contiguous");
  const int64_t want[4] = {B, H, S, D};
  for (int i = 0; i < 4; ++i)
    TORCH_CHECK(want[i] < 0 || t.size(i) == want[i], name, " must have size ",
                want[i], " in dimension ", i, ", got ", t.size(i));
}

// a [B, H, S, D] view (check_bhsd first) whose every row starts on a 16-byte
// boundary, for kernels that read rows with 16-byte loads through arbitrary
// strides: an aligned base and batch/head/seq strides that are multiples of
// 8 elements.  The stride of a dimension of size 1 is never multiplied by a
// non-zero index, so it is free.
void check_rows_aligned16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.const_data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
  for (int i = 0; i < 3; ++i)
    TORCH_CHECK(t.size(i) <= 1 || t.stride(i) % 8 == 0, name,
                ": the stride of dimension ", i,
                " must be a multiple of 8 elements, got ", t.stride(i));
}

// 2-D bf16 rows [N, W], W a positive multiple of 8, at a 16-byte-aligned
// address: the vocab-shard CE and MoE entries, whose callers promise the
// alignment.  Returns (N, W).
std::pair<int64_t, int64_t> check_aligned_rows(const at::Tensor& t,
                                               const char* name,
                                               const at::Tensor& first) {
  auto dims = check_rows(t, name, 8, first);
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.const_data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
  return dims;
}

// Deterministic column-partial stripe count of the dbias kernels: enough
// (stripes x 2048-column blocks) blocks to fill 256 CUs, bounded by the row
// count.  The result fixes the summation order of dbias.  (LayerNorm's is
// layer_norm_bwd_stripes, next to its kernels.)
int stripes_for(int64_t N, int64_t cols) {
  int64_t chunks = std::max<int64_t>(1, cols / 2048);
  int64_t p = std::max<int64_t>(64, 2048 / chunks);
  return (int)std::min<int64_t>({p, N, 512});
}

// the optional trailing out_dtype of the column reductions: fp32 (default)
// or bf16
at::ScalarType check_out_dtype(const c10::optional<at::ScalarType>& dtype) {
  const at::ScalarType t = dtype.value_or(at::kFloat);
  TORCH_CHECK(t == at::kFloat || t == at::kBFloat16,
              "out_dtype must be fp32 or bf16, got ", dtype_name(t));
  return t;
}

// out [F] (and out_b) = the stripe partials [P, F] summed over P on the
// device, in a fixed order, written in out's dtype (check_out_dtype)
void colsum_finalize(const at::Tensor& part, const at::Tensor* part_b,
                     at::Tensor& out, at::Tensor* out_b) {
  HIP_OK(launch_colsum_finalize(
      (const float*)part.const_data_ptr(),
      part_b != nullptr ? (const float*)part_b->const_data_ptr() : nullptr,
      out.mutable_data_ptr(),
      out_b != nullptr ? out_b->mutable_data_ptr() : nullptr,
      (int)part.size(0), part.size(1),
      out.scalar_type() == at::kBFloat16 ? 1 : 0, cur_stream()));
}

// ------------------------------- LayerNorm -------------------------------

std::vector<at::Tensor> layer_norm_fwd(const at::Tensor& x,
                                       const at::Tensor& w,
                                       const at::Tensor& b, double eps) {
  auto [N, H] = check_rows(x, "x", 8, x);
  check_vec(w, "w", at::kBFloat16, H, x);
  check_vec(b, "b", at::kBFloat16, H, x);
  auto y = at::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  auto mean = at::empty({N}, f32);
  auto rstd = at::empty({N}, f32);
  HIP_OK(launch_layer_norm_fwd(x.const_data_ptr(), w.const_data_ptr(),
                               b.const_data_ptr(), y.mutable_data_ptr(),
                               (float*)mean.mutable_data_ptr(),
                               (float*)rstd.mutable_data_ptr(), N, H,
                               (float)eps, cur_stream()));
  return {y, mean, rstd};
}

// Both LayerNorm backwards: `x` (named x_name in refusals) is the normalized
// input, dh the residual gradient or null.  dx and the dw/db stripe partials
// come from launch_layer_norm_bwd, dw and db from one finalize launch, in
// out_dtype.
std::vector<at::Tensor> layer_norm_bwd_common(
    const at::Tensor& dy, const at::Tensor* dh, const at::Tensor& x,
    const char* x_name, const at::Tensor& w, const at::Tensor& mean,
    const at::Tensor& rstd, const c10::optional<at::ScalarType>& out_dtype) {
  auto [N, H] = check_rows(x, x_name, 8, x);
  check_like(dy, "dy", x, x_name);
  if (dh != nullptr) check_like(*dh, "dh", x, x_name);
  check_vec(w, "w", at::kBFloat16, H, x);
  check_vec(mean, "mean", at::kFloat, N, x);
  check_vec(rstd, "rstd", at::kFloat, N, x);
  const at::ScalarType odt = check_out_dtype(out_dtype);
  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto dw = at::empty({H}, x.options().dtype(odt));
  auto db = at::empty({H}, x.options().dtype(odt));
  const int kStripes = layer_norm_bwd_stripes(N, H);
  auto dw_part = at::empty({kStripes, H}, f32);
  auto db_part = at::empty({kStripes, H}, f32);
  if (N > 0) {
    HIP_OK(launch_layer_norm_bwd(
        dy.const_data_ptr(), dh != nullptr ? dh->const_data_ptr() : nullptr,
        x.const_data_ptr(), w.const_data_ptr(),
        (const float*)mean.const_data_ptr(),
        (const float*)rstd.const_data_ptr(), dx.mutable_data_ptr(),
        (float*)dw_part.mutable_data_ptr(),
        (float*)db_part.mutable_data_ptr(), N, H, cur_stream()));
  }
  colsum_finalize(dw_part, &db_part, dw, &db);
  return {dx, dw, db};
}

std::vector<at::Tensor> layer_norm_bwd(
    const at::Tensor& dy, const at::Tensor& x, const at::Tensor& w,
    const at::Tensor& mean, const at::Tensor& rstd,
    const c10::optional<at::ScalarType>& out_dtype) {
  return layer_norm_bwd_common(dy, nullptr, x, "x", w, mean, rstd, out_dtype);
}

// --------------------------- Add + LayerNorm -----------------------------

std::vector<at::Tensor> add_layer_norm_fwd(const at::Tensor& a,
                                           const c10::optional<at::Tensor>& b,
                                           const at::Tensor& w,
                                           const at::Tensor& bias,
                                           double eps) {
  auto [N, H] = check_rows(a, "a", 8, a);
  if (b.has_value()) check_like(*b, "b", a, "a");
  check_vec(w, "w", at::kBFloat16, H, a);
  check_vec(bias, "bias", at::kBFloat16, H, a);
  auto h = at::empty_like(a);
  auto y = at::empty_like(a);
  auto f32 = a.options().dtype(at::kFloat);
  auto mean = at::empty({N}, f32);
  auto rstd = at::empty({N}, f32);
  const void* bp = b.has_value() ? b->const_data_ptr() : nullptr;
  HIP_OK(launch_add_layer_norm_fwd(
      a.const_data_ptr(), bp, w.const_data_ptr(), bias.const_data_ptr(),
      h.mutable_data_ptr(), y.mutable_data_ptr(),
      (float*)mean.mutable_data_ptr(), (float*)rstd.mutable_data_ptr(), N,
      H, (float)eps, cur_stream()));
  return {h, y, mean, rstd};
}

std::vector<at::Tensor> add_layer_norm_bwd(
    const at::Tensor& dy, const c10::optional<at::Tensor>& dh,
    const at::Tensor& h, const at::Tensor& w, const at::Tensor& mean,
    const at::Tensor& rstd, const c10::optional<at::ScalarType>& out_dtype) {
  return layer_norm_bwd_common(dy, dh.has_value() ? &*dh : nullptr, h, "h", w,
                               mean, rstd, out_dtype);
}

// ------------------------------- BiasGelu --------------------------------

at::Tensor bias_gelu_fwd(const at::Tensor& x, const at::Tensor& bias) {
  auto [N, F] = check_rows(x, "x", 8, x);
  check_vec(bias, "bias", at::kBFloat16, F, x);
  auto y = at::empty_like(x);
  HIP_OK(launch_bias_gelu_fwd(x.const_data_ptr(), bias.const_data_ptr(),
                              y.mutable_data_ptr(), N, F, cur_stream()));
  return y;
}

// (dx, dbias): dbias is the column sum of the returned (rounded) dx
std::vector<at::Tensor> bias_gelu_bwd(
    const at::Tensor& dy, const at::Tensor& x, const at::Tensor& bias,
    const c10::optional<at::ScalarType>& out_dtype) {
  auto [N, F] = check_rows(x, "x", 8, x);
  check_like(dy, "dy", x, "x");
  check_vec(bias, "bias", at::kBFloat16, F, x);
  const at::ScalarType odt = check_out_dtype(out_dtype);
  auto dx = at::empty_like(x);
  const int kStripes = stripes_for(N, F);
  auto db = at::empty({F}, x.options().dtype(odt));
  auto db_part = at::empty({kStripes, F}, x.options().dtype(at::kFloat));
  if (N > 0) {
    HIP_OK(launch_bias_gelu_bwd(dy.const_data_ptr(), x.const_data_ptr(),
                                bias.const_data_ptr(), dx.mutable_data_ptr(),
                                (float*)db_part.mutable_data_ptr(), N, F,
                                kStripes, cur_stream()));
  }
  colsum_finalize(db_part, nullptr, db, nullptr);
  return {dx, db};
}

// column sum of a bf16 [N, F] tensor -> [F] in out_dtype (striped partials +
// finalize): the bias-gradient reduction for plain +bias layers (the
// at::native reduce path cost ~8 ms/step in the r2 profile)
at::Tensor colsum_bf16(const at::Tensor& t,
                       const c10::optional<at::ScalarType>& out_dtype) {
  // any positive width: the kernels have a scalar tail
  auto [N, F] = check_rows(t, "t", 1, t);
  const at::ScalarType odt = check_out_dtype(out_dtype);
  const int kStripes = stripes_for(N, F);
  auto part = at::empty({kStripes, F}, t.options().dtype(at::kFloat));
  auto out = at::empty({F}, t.options().dtype(odt));
  if (N > 0) {
    HIP_OK(launch_colsum_partial(t.const_data_ptr(),
                                 (float*)part.mutable_data_ptr(), N, F,
                                 kStripes, cur_stream()));
  }
  colsum_finalize(part, nullptr, out, nullptr);
  return out;
}

// ----------------------------- skinny GEMM -------------------------------

// y[M,N] bf16 = x[M,K] @ Wp^T (+ bias) for decode-shaped M<=64; wp is
// the packed [K/8, N, 8] layout (bf16 or e4m3 — pass wscale for e4m3).
// Two launches: split-K partials then a deterministic finalize
// (reduce + bias + cast) — no zero-fill, no atomics.
at::Tensor skinny_gemm(const at::Tensor& wp, const at::Tensor& x,
                       const c10::optional<at::Tensor>& wscale,
                       const c10::optional<at::Tensor>& bias,
                       int64_t N, int64_t K, int64_t splits) {
  TORCH_CHECK(N > 0 && N % 64 == 0, "N must be a positive multiple of 64");
  TORCH_CHECK(K > 0 && K % 64 == 0, "K must be a positive multiple of 64");
  const bool fp8 = wscale.has_value();
  if (fp8) {
    check_device(wp, "wp", wp);
    TORCH_CHECK(wp.element_size() == 1,
                "wp must hold one-byte elements when wscale is given");
    TORCH_CHECK(wp.is_contiguous() && wp.numel() == N * K,
                "wp must be contiguous with N*K elements");
    check_vec(*wscale, "wscale", at::kFloat, 1, wp);
  } else {
    check_vec(wp, "wp", at::kBFloat16, N * K, wp);
  }
  if (bias.has_value()) check_vec(*bias, "bias", at::kBFloat16, N, wp);
  auto [M, Kx] = check_rows(x, "x", 64, wp);
  TORCH_CHECK(x.dim() == 2 && Kx == K, "x must be [M, K]");
  TORCH_CHECK(M >= 1 && M <= 64, "skinny path is for M <= 64");
  int64_t MT = 4;
  while (MT < M) MT *= 2;
  // what the kernel's 8-deep pipeline and its 64 KB LDS x-slice take
  TORCH_CHECK(splits >= 1 && (K / 64) % splits == 0 &&
                  (K / 8 / splits) * 16 * MT <= 65536,
              "splits must divide K/64 and leave (K/8/splits)*16*MT <= 65536");
  at::Tensor xp = x;
  if (MT != M) {
    xp = at::zeros({MT, K}, x.options());
    xp.narrow(0, 0, M).copy_(x);
  }
  auto part = at::empty({splits, MT, N}, x.options().dtype(at::kFloat));
  auto y = at::empty({M, N}, x.options());
  HIP_OK(launch_skinny_gemm(
      wp.const_data_ptr(), xp.const_data_ptr(),
      (float*)part.mutable_data_ptr(),
      bias.has_value() ? bias->const_data_ptr() : nullptr,
      y.mutable_data_ptr(),
      fp8 ? (const float*)wscale->const_data_ptr() : nullptr, M, MT, N, K,
      (int)splits, fp8 ? 1 : 0, cur_stream()));
  return y;
}

// -------------------------------- AdamW ----------------------------------

void adamw_step_raw(const at::Tensor& descs, const at::Tensor& chunks,
                    int64_t step, double lr, double beta1, double beta2,
                    double eps, double weight_decay, double grad_scale,
                    const c10::optional<at::Tensor>& grad_sumsq,
                    double max_grad_norm) {
  TORCH_CHECK(descs.dim() == 2 && descs.size(1) == 6, "descs must be [n, 6]");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 2,
              "chunks must be [m, 2]");
  check_vec(descs, "descs", at::kLong, descs.numel(), descs);
  check_vec(chunks, "chunks", at::kInt, chunks.numel(), descs);
  const float* sumsq = nullptr;
  if (grad_sumsq.has_value()) {
    check_vec(*grad_sumsq, "grad_sumsq", at::kFloat, 1, descs);
    TORCH_CHECK(max_grad_norm > 0, "max_grad_norm must be positive");
    sumsq = (const float*)grad_sumsq->const_data_ptr();
  }
  HIP_OK(launch_adamw(descs.const_data_ptr(), chunks.const_data_ptr(),
                      (int)chunks.size(0), (float)lr, (float)beta1,
                      (float)beta2, (float)eps, (float)weight_decay,
                      (float)grad_scale, (int)step, sumsq,
                      (float)max_grad_norm, cur_stream()));
}

// descs/chunks: the AdamW tables (only g, numel and is_bf16 are read);
// partials: fp32 workspace [num_chunks]; out: fp32 [1]
void multi_tensor_sumsq_raw(const at::Tensor& descs, const at::Tensor& chunks,
                            at::Tensor& partials, at::Tensor& out) {
  TORCH_CHECK(descs.dim() == 2 && descs.size(1) == 6, "descs must be [n, 6]");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 2,
              "chunks must be [m, 2]");
  check_vec(descs, "descs", at::kLong, descs.numel(), descs);
  check_vec(chunks, "chunks", at::kInt, chunks.numel(), descs);
  int64_t n = chunks.size(0);
  // the workspace may be longer than the chunk table
  check_typed(partials, "partials", at::kFloat, descs);
  TORCH_CHECK(partials.is_contiguous() && partials.numel() >= n,
              "partials must be contiguous with at least num_chunks elements");
  check_vec(out, "out", at::kFloat, 1, descs);
  HIP_OK(launch_multi_tensor_sumsq(
      descs.const_data_ptr(), chunks.const_data_ptr(), (int)n,
      (float*)partials.mutable_data_ptr(), (float*)out.mutable_data_ptr(),
      cur_stream()));
}

// ----------------------------- CrossEntropy ------------------------------

std::vector<at::Tensor> cross_entropy_fwd(const at::Tensor& logits,
                                          const at::Tensor& targets) {
  auto [N, V] = check_rows(logits, "logits", 8, logits);
  check_vec(targets, "targets", at::kLong, N, logits);
  auto f32 = logits.options().dtype(at::kFloat);
  auto loss = at::empty({N}, f32);
  auto lse = at::empty({N}, f32);
  HIP_OK(launch_ce_fwd(logits.const_data_ptr(),
                       (const int64_t*)targets.const_data_ptr(),
                       (float*)loss.mutable_data_ptr(),
                       (float*)lse.mutable_data_ptr(), N, V, cur_stream()));
  return {loss, lse};
}

at::Tensor cross_entropy_bwd(const at::Tensor& dloss, const at::Tensor& logits,
                             const at::Tensor& targets,
                             const at::Tensor& lse) {
  auto [N, V] = check_rows(logits, "logits", 8, logits);
  check_vec(targets, "targets", at::kLong, N, logits);
  check_vec(lse, "lse", at::kFloat, N, logits);
  // any dtype and layout: converted below
  check_device(dloss, "dloss", logits);
  TORCH_CHECK(dloss.numel() == N, "dloss must have ", N, " elements, got ",
              dloss.numel());
  auto dlogits = at::empty_like(logits);
  auto dl = dloss.to(at::kFloat).contiguous();
  HIP_OK(launch_ce_bwd((const float*)dl.const_data_ptr(), logits.const_data_ptr(),
                       (const int64_t*)targets.const_data_ptr(),
                       (const float*)lse.const_data_ptr(),
                       dlogits.mutable_data_ptr(), N, V, 0, cur_stream()));
  return dlogits;
}

// One rank's vocab shard: logits bf16 [N, Vs] = global columns
// [vocab_start, vocab_start + Vs), targets int64 [N] of global vocab ids.
at::Tensor cross_entropy_partial_fwd(const at::Tensor& logits,
                                     const at::Tensor& targets,
                                     int64_t vocab_start) {
  auto [N, V] = check_aligned_rows(logits, "logits", logits);
  check_vec(targets, "targets", at::kLong, N, logits);
  TORCH_CHECK(vocab_start >= 0, "vocab_start must be >= 0");
  auto stats = at::empty({3, N}, logits.options().dtype(at::kFloat));
  HIP_OK(launch_ce_partial_fwd(logits.const_data_ptr(),
                               (const int64_t*)targets.const_data_ptr(),
                               (float*)stats.mutable_data_ptr(), N, V,
                               vocab_start, cur_stream()));
  return stats;
}

at::Tensor cross_entropy_shard_bwd(const at::Tensor& dloss,
                                   const at::Tensor& logits,
                                   const at::Tensor& targets,
                                   const at::Tensor& lse,
                                   int64_t vocab_start) {
  auto [N, V] = check_aligned_rows(logits, "logits", logits);
  check_vec(targets, "targets", at::kLong, N, logits);
  TORCH_CHECK(vocab_start >= 0, "vocab_start must be >= 0");
  check_vec(lse, "lse", at::kFloat, N, logits);
  // any dtype and layout: converted below
  check_device(dloss, "dloss", logits);
  TORCH_CHECK(dloss.numel() == N, "dloss must have ", N, " elements, got ",
              dloss.numel());
  auto dlogits = at::empty_like(logits);
  auto dl = dloss.to(at::kFloat).contiguous();
  HIP_OK(launch_ce_bwd((const float*)dl.const_data_ptr(),
                       logits.const_data_ptr(),
                       (const int64_t*)targets.const_data_ptr(),
                       (const float*)lse.const_data_ptr(),
                       dlogits.mutable_data_ptr(), N, V, vocab_start,
                       cur_stream()));
  return dlogits;
}

// ------------------------------ Attention --------------------------------

// q/k/v/o are logical [B, H, S, D] views with arbitrary B/H/S strides and a
// contiguous D — so the packed qkv layout [B, S, heads, 3*D] feeds the
// kernel directly, with no permute/contiguous copies on the hot path.

// The launchers' stride array: (batch, head, seq) strides of each 4-D
// tensor, three entries per tensor in argument order.
template <typename... T>
std::array<int64_t, 3 * sizeof...(T)> bhs_strides(const T&... t) {
  std::array<int64_t, 3 * sizeof...(T)> s;
  int64_t* p = s.data();
  ((*p++ = t.stride(0), *p++ = t.stride(1), *p++ = t.stride(2)), ...);
  return s;
}

// optional operand: is it there, and its data pointer or nullptr
bool given(const c10::optional<at::Tensor>& t) {
  return t.has_value() && t->defined();
}

const void* opt_ptr(const c10::optional<at::Tensor>& t) {
  return given(t) ? t->const_data_ptr() : nullptr;
}

// The inputs every fused attention entry takes: q [B,H,S,D]; k and v
// [B,H,Skv,D] (S != Skv is legal: ring attention, cached decode); optional
// ALiBi slopes fp32 [H] and per-batch real KV lengths int32 [B] (continuous
// batching decode; elements past a slot's length are masked).  head_dim is
// a multiple of 16 up to max_D, up to 128 with slopes or lengths.
void check_attn_inputs(const at::Tensor& q, const at::Tensor& k,
                       const at::Tensor& v,
                       const c10::optional<at::Tensor>& alibi,
                       const c10::optional<at::Tensor>& kv_lens,
                       int64_t max_D) {
  check_bhsd(q, "q", -1, -1, -1, -1, q);
  const int64_t B = q.size(0), H = q.size(1), D = q.size(3);
  check_bhsd(k, "k", B, H, -1, D, q);
  check_bhsd(v, "v", B, H, k.size(2), D, q);
  TORCH_CHECK(D > 0 && D % 16 == 0 && D <= max_D,
              "head_dim must be a multiple of 16 up to ", max_D, ", got ", D);
  TORCH_CHECK(D <= 128 || !(given(alibi) || given(kv_lens)),
              "alibi and kv_lens need head_dim <= 128, got ", D);
  if (given(alibi)) check_vec(*alibi, "alibi", at::kFloat, H, q);
  if (given(kv_lens)) check_vec(*kv_lens, "kv_lens", at::kInt, B, q);
}

at::Tensor attn_fwd_out(const at::Tensor& q, const at::Tensor& k,
                        const at::Tensor& v, at::Tensor o, at::Tensor lse,
                        bool causal, double scale,
                        const c10::optional<at::Tensor>& alibi =
                            c10::nullopt,
                        const c10::optional<at::Tensor>& kv_lens =
                            c10::nullopt) {
  check_attn_inputs(q, k, v, alibi, kv_lens, 256);
  int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  int64_t Skv = k.size(2);
  check_bhsd(o, "o", B, H, S, D, q);
  check_vec(lse, "lse", at::kFloat, B * H * S, q);
  const auto strides = bhs_strides(q, k, v, o);
  HIP_OK(launch_attn_fwd(q.const_data_ptr(), k.const_data_ptr(),
                         v.const_data_ptr(), o.mutable_data_ptr(),
                         (float*)lse.mutable_data_ptr(), B, H, S, Skv, D,
                         (float)scale, causal ? 1 : 0,
                         (const float*)opt_ptr(alibi),
                         (const int*)opt_ptr(kv_lens), strides.data(),
                         cur_stream()));
  return o;
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k,
                                 const at::Tensor& v, bool causal,
                                 double scale,
                                 const c10::optional<at::Tensor>& alibi =
                                     c10::nullopt,
                                 const c10::optional<at::Tensor>& kv_lens =
                                     c10::nullopt) {
  // before the allocations; attn_fwd_out repeats it, which costs nothing
  check_attn_inputs(q, k, v, alibi, kv_lens, 256);
  int64_t B = q.size(0), H = q.size(1), S = q.size(2);
  auto o = at::empty_like(q.contiguous());
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  attn_fwd_out(q, k, v, o, lse, causal, scale, alibi, kv_lens);
  return {o, lse};
}

// Split-KV decode attention (attention_decode.hip): one query row per
// (batch, head), non-causal over the first kv_lens[b] (or Skv) keys.
// q [B,H,1,D], k and v [B,H,Skv,D] views as above, with 16-byte-aligned
// rows; head_dim any multiple of 16 up to 256, with or without slopes and
// lengths.  Returns (o [B,H,1,D] bf16, lse [B,H,1] fp32).  The workspace is
// an ordinary allocation on the current stream, so the op can be captured.
std::vector<at::Tensor> attn_decode(const at::Tensor& q, const at::Tensor& k,
                                    const at::Tensor& v, double scale,
                                    const c10::optional<at::Tensor>& alibi =
                                        c10::nullopt,
                                    const c10::optional<at::Tensor>& kv_lens =
                                        c10::nullopt) {
  check_bhsd(q, "q", -1, -1, -1, -1, q);
  const int64_t B = q.size(0), H = q.size(1), D = q.size(3);
  TORCH_CHECK(q.size(2) == 1, "q must hold one query row per head, got ",
              q.size(2));
  check_bhsd(k, "k", B, H, -1, D, q);
  const int64_t Skv = k.size(2);
  check_bhsd(v, "v", B, H, Skv, D, q);
  TORCH_CHECK(D > 0 && D % 16 == 0 && D <= 256,
              "head_dim must be a multiple of 16 up to 256, got ", D);
  // (batch, head) pairs ride on grid.y
  TORCH_CHECK(B * H <= 65535, "q: at most 65535 (batch, head) pairs, got ",
              B * H);
  if (given(alibi)) check_vec(*alibi, "alibi", at::kFloat, H, q);
  if (given(kv_lens)) check_vec(*kv_lens, "kv_lens", at::kInt, B, q);
  check_rows_aligned16(q, "q");
  check_rows_aligned16(k, "k");
  check_rows_aligned16(v, "v");
  auto f32 = q.options().dtype(at::kFloat);
  auto o = at::empty({B, H, 1, D}, q.options());
  auto lse = at::empty({B, H, 1}, f32);
  if (B * H == 0) return {o, lse};
  auto ws = at::empty({attn_decode_workspace_floats(B, H, Skv, D)}, f32);
  const auto strides = bhs_strides(q, k, v, o);
  HIP_OK(launch_attn_decode(q.const_data_ptr(), k.const_data_ptr(),
                            v.const_data_ptr(), o.mutable_data_ptr(),
                            (float*)lse.mutable_data_ptr(),
                            (float*)ws.mutable_data_ptr(), B, H, Skv, D,
                            (float)scale, (const float*)opt_ptr(alibi),
                            (const int*)opt_ptr(kv_lens), strides.data(),
                            cur_stream()));
  return {o, lse};
}

// Blocked attention forward for head_dim > 128 (the fused kernel tiles
// head_dim in registers up to 128): q-block loop, scores via bf16
// hipBLASLt GEMMs, fp32 softmax, never materializes more than one
// [Bq, Skv] block.  Serves CodeGen-6B/16B-class models (head_dim 256).
std::vector<at::Tensor> attn_fwd_blocked(const at::Tensor& q_,
                                         const at::Tensor& k_,
                                         const at::Tensor& v_, bool causal,
                                         double scale) {
  auto q = q_.contiguous(), k = k_.contiguous(), v = v_.contiguous();
  int64_t B = q.size(0), H = q.size(1), S = q.size(2);
  int64_t Skv = k.size(2);
  auto o = at::empty_like(q);
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  const int64_t BQ = 256;
  int64_t qoff = Skv - S;  // cached decode: q global position offset
  for (int64_t qs = 0; qs < S; qs += BQ) {
    int64_t qe = std::min(qs + BQ, S);
    auto qb = q.slice(2, qs, qe);
    int64_t ke = causal ? std::min(qe + qoff, Skv) : Skv;
    auto kb = k.slice(2, 0, ke);
    auto s_blk = at::matmul(qb, kb.transpose(-1, -2)).to(at::kFloat)
                     .mul_(scale);
    if (causal) {
      // mask j > i + qoff
      auto qi = at::arange(qs + qoff, qe + qoff, q.options().dtype(at::kLong));
      auto kj = at::arange(ke, q.options().dtype(at::kLong));
      auto mask = kj.view({1, 1, 1, ke}) > qi.view({1, 1, qe - qs, 1});
      s_blk.masked_fill_(mask, -std::numeric_limits<float>::infinity());
    }
    auto m = std::get<0>(s_blk.max(-1, true));
    auto p = at::exp(s_blk - m);
    auto l = p.sum(-1, true);
    o.slice(2, qs, qe).copy_(
        at::matmul((p / l).to(at::kBFloat16), v.slice(2, 0, ke)));
    lse.slice(2, qs, qe).copy_((m + at::log(l)).squeeze(-1));
  }
  return {o, lse};
}

// Attention backward: deterministic blocked recompute; all GEMMs in bf16
// (hipBLASLt / MFMA), softmax math in fp32.  The q-block loop keeps the
// S x S score matrix from materializing beyond one [Bq, Skv] block.
// (A fully hand-written HIP bwd kernel replaces this on the optimization
// path.)
std::vector<at::Tensor> attn_bwd_blocked(const at::Tensor& dout_, const at::Tensor& q_,
                                 const at::Tensor& k_, const at::Tensor& v_,
                                 const at::Tensor& o_, const at::Tensor& lse,
                                 bool causal, double scale) {
  auto q = q_.contiguous(), k = k_.contiguous(), v = v_.contiguous();
  auto dout = dout_.contiguous(), o = o_.contiguous();
  int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  int64_t Skv = k.size(2);
  auto dq = at::empty_like(q);
  auto dk = at::zeros_like(k, k.options().dtype(at::kFloat));
  auto dv = at::zeros_like(v, v.options().dtype(at::kFloat));
  // delta = rowsum(dO * O), fp32, computed once
  auto delta = (dout.to(at::kFloat) * o.to(at::kFloat)).sum(-1, true);
  auto lse4 = lse.view({B, H, S, 1});
  const int64_t BQ = 256;
  for (int64_t qs = 0; qs < S; qs += BQ) {
    int64_t qe = std::min(qs + BQ, S);
    auto qb = q.slice(2, qs, qe);
    auto dob = dout.slice(2, qs, qe);
    int64_t ke = causal ? std::min(qe, Skv) : Skv;
    auto kb = k.slice(2, 0, ke);
    auto vb = v.slice(2, 0, ke);
    // p = exp(s*scale - lse), zeroed above the causal diagonal via tril
    auto s = at::matmul(qb, kb.transpose(-1, -2));  // bf16 GEMM
    auto p = at::exp(s.to(at::kFloat) * scale - lse4.slice(2, qs, qe));
    if (causal) p = p.tril_(qs);
    auto p_bf = p.to(at::kBFloat16);
    dv.slice(2, 0, ke).add_(at::matmul(p_bf.transpose(-1, -2), dob));
    auto dp = at::matmul(dob, vb.transpose(-1, -2));  // bf16 GEMM
    auto ds = p.mul_(dp.to(at::kFloat) - delta.slice(2, qs, qe))
                  .mul_(scale);  // reuse p storage
    auto ds_bf = ds.to(at::kBFloat16);
    dq.slice(2, qs, qe).copy_(at::matmul(ds_bf, kb));
    dk.slice(2, 0, ke).add_(at::matmul(ds_bf.transpose(-1, -2), qb));
  }
  return {dq, dk.to(k.scalar_type()), dv.to(v.scalar_type())};
}

// Hand-written flash-attention backward (gfx950 MFMA, deterministic
// two-kernel split).  All tensors are logical [B,H,S,D] views with
// arbitrary B/H/S strides (contiguous D) — dq/dk/dv may be strided views
// into a packed dqkv buffer.
// dout, o [B,H,S,D] and the forward's lse, fp32 with B*H*S elements.
// head_dim <= 128 as in the fused forward with the same operands, so no
// o/lse pair exists for a wider head.
void check_attn_bwd_inputs(const at::Tensor& dout, const at::Tensor& q,
                           const at::Tensor& k, const at::Tensor& v,
                           const at::Tensor& o, const at::Tensor& lse,
                           const c10::optional<at::Tensor>& alibi) {
  check_attn_inputs(q, k, v, alibi, c10::nullopt, 128);
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  check_bhsd(dout, "dout", B, H, S, D, q);
  check_bhsd(o, "o", B, H, S, D, q);
  check_typed(lse, "lse", at::kFloat, q);
  TORCH_CHECK(lse.numel() == B * H * S, "lse must have ", B * H * S,
              " elements, got ", lse.numel());
}

void attn_bwd_out(const at::Tensor& dout, const at::Tensor& q,
                  const at::Tensor& k, const at::Tensor& v,
                  const at::Tensor& o, const at::Tensor& lse, at::Tensor dq,
                  at::Tensor dk, at::Tensor dv, bool causal, double scale,
                  const c10::optional<at::Tensor>& alibi = c10::nullopt) {
  check_attn_bwd_inputs(dout, q, k, v, o, lse, alibi);
  int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  int64_t Skv = k.size(2);
  check_bhsd(dq, "dq", B, H, S, D, q);
  check_bhsd(dk, "dk", B, H, Skv, D, q);
  check_bhsd(dv, "dv", B, H, Skv, D, q);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  auto lse_c = lse.contiguous();
  const auto strides = bhs_strides(q, k, v, dout, dq, dk, dv, o);
  HIP_OK(launch_attn_bwd(q.const_data_ptr(), k.const_data_ptr(),
                         v.const_data_ptr(), o.const_data_ptr(),
                         dout.const_data_ptr(),
                         (const float*)lse_c.const_data_ptr(),
                         (float*)delta.mutable_data_ptr(),
                         dq.mutable_data_ptr(), dk.mutable_data_ptr(),
                         dv.mutable_data_ptr(), B, H, S, Skv, D,
                         (float)scale, causal ? 1 : 0,
                         (const float*)opt_ptr(alibi), strides.data(),
                         cur_stream()));
}

std::vector<at::Tensor> attn_bwd(const at::Tensor& dout, const at::Tensor& q,
                                 const at::Tensor& k, const at::Tensor& v,
                                 const at::Tensor& o, const at::Tensor& lse,
                                 bool causal, double scale,
                                 const c10::optional<at::Tensor>& alibi =
                                     c10::nullopt) {
  // before the allocations; attn_bwd_out repeats it, which costs nothing
  check_attn_bwd_inputs(dout, q, k, v, o, lse, alibi);
  auto dq = at::empty_like(q.contiguous());
  auto dk = at::empty_like(k.contiguous());
  auto dv = at::empty_like(v.contiguous());
  attn_bwd_out(dout, q, k, v, o, lse, dq, dk, dv, causal, scale, alibi);
  return {dq, dk, dv};
}

// ------------------------------ MoE routing ------------------------------

constexpr int64_t kMoeMaxTokens = int64_t(1) << 30;

// logits [N, E] bf16 -> (w1, w2, idx1, idx2, slot1, slot2, src, aux,
// count1); every shape depends on (N, E, C) only and nothing is read back
std::vector<at::Tensor> moe_route_fwd(const at::Tensor& logits,
                                      int64_t capacity) {
  auto [N, E] = check_rows(logits, "logits", 1, logits);
  TORCH_CHECK(logits.dim() == 2, "logits must be [N, E]");
  const int64_t C = capacity;
  TORCH_CHECK(E >= 2 && E <= 128, "num_experts must be in [2, 128], got ", E);
  TORCH_CHECK(C >= 1, "capacity must be >= 1");
  TORCH_CHECK(C < (int64_t(1) << 31) / E, "E * capacity must be < 2^31");
  TORCH_CHECK(N <= kMoeMaxTokens, "at most 2^30 tokens");
  auto f32 = logits.options().dtype(at::kFloat);
  auto i32 = logits.options().dtype(at::kInt);
  auto w1 = at::empty({N}, f32), w2 = at::empty({N}, f32);
  auto idx1 = at::empty({N}, i32), idx2 = at::empty({N}, i32);
  auto slot1 = at::empty({N}, i32), slot2 = at::empty({N}, i32);
  if (N == 0) {
    return {w1, w2, idx1, idx2, slot1, slot2, at::full({E * C}, -1, i32),
            at::zeros({}, f32), at::zeros({E}, i32)};
  }
  auto src = at::empty({E * C}, i32);
  auto aux = at::empty({}, f32);
  auto count1 = at::empty({E}, i32);
  const int64_t nblocks = (N + 255) / 256;
  auto hist = at::empty({2, nblocks, E}, i32);
  auto ppart = at::empty({nblocks, E}, f32);
  auto psum = at::empty({E}, f32);
  int* hist1 = (int*)hist.mutable_data_ptr();
  int* hist2 = hist1 + nblocks * E;
  HIP_OK(launch_moe_route(
      logits.const_data_ptr(), (float*)w1.mutable_data_ptr(),
      (float*)w2.mutable_data_ptr(), (int*)idx1.mutable_data_ptr(),
      (int*)idx2.mutable_data_ptr(), (int*)slot1.mutable_data_ptr(),
      (int*)slot2.mutable_data_ptr(), hist1, hist2,
      (float*)ppart.mutable_data_ptr(), N, E, cur_stream()));
  at::sum_out(psum, ppart, {0});
  HIP_OK(launch_moe_slots(
      (const int*)idx1.const_data_ptr(), (const int*)idx2.const_data_ptr(),
      hist1, hist2, (const float*)psum.const_data_ptr(),
      (int*)count1.mutable_data_ptr(), (float*)aux.mutable_data_ptr(),
      (int*)slot1.mutable_data_ptr(), (int*)slot2.mutable_data_ptr(),
      (int*)src.mutable_data_ptr(), N, E, C, cur_stream()));
  return {w1, w2, idx1, idx2, slot1, slot2, src, aux, count1};
}

at::Tensor moe_route_bwd(const at::Tensor& logits, const at::Tensor& idx1,
                         const at::Tensor& idx2, const at::Tensor& w1,
                         const at::Tensor& w2, const at::Tensor& count1,
                         const at::Tensor& dw1, const at::Tensor& dw2,
                         const at::Tensor& daux) {
  auto [N, E] = check_rows(logits, "logits", 1, logits);
  TORCH_CHECK(logits.dim() == 2, "logits must be [N, E]");
  TORCH_CHECK(E >= 2 && E <= 128, "num_experts must be in [2, 128], got ", E);
  TORCH_CHECK(N <= kMoeMaxTokens, "at most 2^30 tokens");
  check_vec(idx1, "idx1", at::kInt, N, logits);
  check_vec(idx2, "idx2", at::kInt, N, logits);
  check_vec(count1, "count1", at::kInt, E, logits);
  check_vec(w1, "w1", at::kFloat, N, logits);
  check_vec(w2, "w2", at::kFloat, N, logits);
  check_vec(dw1, "dw1", at::kFloat, N, logits);
  check_vec(dw2, "dw2", at::kFloat, N, logits);
  check_vec(daux, "daux", at::kFloat, 1, logits);
  auto dlogits = at::empty_like(logits);
  if (N == 0) return dlogits;
  HIP_OK(launch_moe_route_bwd(
      logits.const_data_ptr(), (const int*)idx1.const_data_ptr(),
      (const int*)idx2.const_data_ptr(), (const float*)w1.const_data_ptr(),
      (const float*)w2.const_data_ptr(), (const int*)count1.const_data_ptr(),
      (const float*)dw1.const_data_ptr(), (const float*)dw2.const_data_ptr(),
      (const float*)daux.const_data_ptr(), dlogits.mutable_data_ptr(), N, E,
      cur_stream()));
  return dlogits;
}

// out[s] = x[src[s]] or zeros.  With (slot1, w1, w2) row s is also scaled
// by the gate weight of the choice that owns it (the combine's dy).
at::Tensor moe_dispatch(const at::Tensor& x, const at::Tensor& src,
                        const c10::optional<at::Tensor>& slot1,
                        const c10::optional<at::Tensor>& w1,
                        const c10::optional<at::Tensor>& w2) {
  auto [N, H] = check_aligned_rows(x, "x", x);
  const int64_t S = src.numel();
  check_vec(src, "src", at::kInt, S, x);
  TORCH_CHECK(S < (int64_t(1) << 31), "E * capacity must be < 2^31");
  TORCH_CHECK(N <= kMoeMaxTokens, "at most 2^30 tokens");
  const bool scaled = slot1.has_value();
  TORCH_CHECK(w1.has_value() == scaled && w2.has_value() == scaled,
              "slot1, w1 and w2 go together");
  if (scaled) {
    check_vec(*slot1, "slot1", at::kInt, N, x);
    check_vec(*w1, "w1", at::kFloat, N, x);
    check_vec(*w2, "w2", at::kFloat, N, x);
  }
  auto out = at::empty({S, H}, x.options());
  if (S == 0) return out;
  HIP_OK(launch_moe_dispatch(
      x.const_data_ptr(), (const int*)src.const_data_ptr(),
      scaled ? (const int*)slot1->const_data_ptr() : nullptr,
      scaled ? (const float*)w1->const_data_ptr() : nullptr,
      scaled ? (const float*)w2->const_data_ptr() : nullptr,
      out.mutable_data_ptr(), S, N, H, cur_stream()));
  return out;
}

// out[t] = w1[t] * y[slot1[t]] + w2[t] * y[slot2[t]] (dropped terms
// skipped); without weights the plain sum (the dispatch's dx)
at::Tensor moe_combine(const at::Tensor& y,
                       const c10::optional<at::Tensor>& w1,
                       const c10::optional<at::Tensor>& w2,
                       const at::Tensor& slot1, const at::Tensor& slot2) {
  auto [S, H] = check_aligned_rows(y, "y", y);
  const int64_t N = slot1.numel();
  TORCH_CHECK(S < (int64_t(1) << 31), "E * capacity must be < 2^31");
  TORCH_CHECK(N <= kMoeMaxTokens, "at most 2^30 tokens");
  check_vec(slot1, "slot1", at::kInt, N, y);
  check_vec(slot2, "slot2", at::kInt, N, y);
  TORCH_CHECK(w1.has_value() == w2.has_value(), "w1 and w2 go together");
  if (w1.has_value()) {
    check_vec(*w1, "w1", at::kFloat, N, y);
    check_vec(*w2, "w2", at::kFloat, N, y);
  }
  auto out = at::empty({N, H}, y.options());
  if (N == 0) return out;
  HIP_OK(launch_moe_combine(
      y.const_data_ptr(),
      w1.has_value() ? (const float*)w1->const_data_ptr() : nullptr,
      w2.has_value() ? (const float*)w2->const_data_ptr() : nullptr,
      (const int*)slot1.const_data_ptr(), (const int*)slot2.const_data_ptr(),
      out.mutable_data_ptr(), N, S, H, cur_stream()));
  return out;
}

// (dw1, dw2)[t] = <dout[t], y[slot_k[t]]> in fp32, 0 when dropped
std::vector<at::Tensor> moe_combine_dw(const at::Tensor& dout,
                                       const at::Tensor& y,
                                       const at::Tensor& slot1,
                                       const at::Tensor& slot2) {
  auto [N, H] = check_aligned_rows(dout, "dout", dout);
  auto [S, Hy] = check_aligned_rows(y, "y", dout);
  TORCH_CHECK(Hy == H, "dout and y must share H");
  TORCH_CHECK(S < (int64_t(1) << 31), "E * capacity must be < 2^31");
  TORCH_CHECK(N <= kMoeMaxTokens, "at most 2^30 tokens");
  check_vec(slot1, "slot1", at::kInt, N, dout);
  check_vec(slot2, "slot2", at::kInt, N, dout);
  auto f32 = dout.options().dtype(at::kFloat);
  auto dw1 = at::empty({N}, f32), dw2 = at::empty({N}, f32);
  if (N == 0) return {dw1, dw2};
  HIP_OK(launch_moe_combine_dw(
      dout.const_data_ptr(), y.const_data_ptr(),
      (const int*)slot1.const_data_ptr(), (const int*)slot2.const_data_ptr(),
      (float*)dw1.mutable_data_ptr(), (float*)dw2.mutable_data_ptr(), N, S,
      H, cur_stream()));
  return {dw1, dw2};
}

// both probes read one 512-element bf16 tile per operand
at::Tensor mfma_probe(const at::Tensor& a, const at::Tensor& b) {
  check_vec(a, "a", at::kBFloat16, 512, a);
  check_vec(b, "b", at::kBFloat16, 512, a);
  auto d = at::empty({16, 16}, a.options().dtype(at::kFloat));
  HIP_OK(launch_mfma_probe(a.const_data_ptr(), b.const_data_ptr(),
                           (float*)d.mutable_data_ptr(), cur_stream()));
  return d;
}

at::Tensor mfma_probe32(const at::Tensor& a, const at::Tensor& b) {
  check_vec(a, "a", at::kBFloat16, 512, a);
  check_vec(b, "b", at::kBFloat16, 512, a);
  auto d = at::empty({32, 32}, a.options().dtype(at::kFloat));
  HIP_OK(launch_mfma_probe32(a.const_data_ptr(), b.const_data_ptr(),
                             (float*)d.mutable_data_ptr(), cur_stream()));
  return d;
}

// fp8 quantize: one-pass amax + delayed-scale cast (optional transposed
// twin for the dW GEMM).  x: bf16 contiguous; scale: fp32 scalar tensor
// on device (previous-step scale); returns (q, qt | empty, amax).
std::vector<at::Tensor> fp8_quantize(const at::Tensor& x,
                                     const at::Tensor& scale, bool dual,
                                     bool e5m2) {
  // any shape: the single-layout kernel runs over the flat elements
  check_vec(x, "x", at::kBFloat16, x.numel(), x);
  check_vec(scale, "scale", at::kFloat, 1, x);
  auto qtype = e5m2 ? at::kFloat8_e5m2 : at::kFloat8_e4m3fn;
  auto amax = at::zeros({1}, x.options().dtype(at::kFloat));
  auto q = at::empty(x.sizes(), x.options().dtype(qtype));
  if (!dual) {
    TORCH_CHECK(x.numel() % 8 == 0, "numel must be divisible by 8");
    HIP_OK(launch_fp8_quantize(x.const_data_ptr(), q.data_ptr(),
                               (const float*)scale.const_data_ptr(),
                               (float*)amax.data_ptr(), x.numel(),
                               e5m2 ? 1 : 0, cur_stream()));
    return {q, at::Tensor(), amax};
  }
  TORCH_CHECK(x.dim() == 2, "dual quantize needs a 2-D tensor");
  int64_t M = x.size(0), N = x.size(1);
  auto qt = at::empty({N, M}, x.options().dtype(qtype));
  HIP_OK(launch_fp8_quantize_dual(x.const_data_ptr(), q.data_ptr(),
                                  qt.data_ptr(),
                                  (const float*)scale.const_data_ptr(),
                                  (float*)amax.data_ptr(), M, N,
                                  e5m2 ? 1 : 0, cur_stream()));
  return {q, qt, amax};
}

// ---------------------- producers fused with quantize ----------------------

// row tiles (64 rows) ride on grid.y, which holds at most 65535
constexpr int64_t kFusedQuantMaxRows = int64_t(1) << 21;

// gelu(x + bias) quantized to e4m3 in both layouts, no bf16 output:
// x [.., F] bf16 -> (q [N, F], qt [F, N], amax [1]), byte-equal to
// bias_gelu_fwd followed by fp8_quantize(y, scale, dual, e4m3)
std::vector<at::Tensor> bias_gelu_fp8(const at::Tensor& x,
                                      const at::Tensor& bias,
                                      const at::Tensor& scale) {
  auto [N, F] = check_rows(x, "x", 8, x);
  TORCH_CHECK(N < kFusedQuantMaxRows, "at most 2^21 rows");
  check_vec(bias, "bias", at::kBFloat16, F, x);
  check_vec(scale, "scale", at::kFloat, 1, x);
  auto q8 = x.options().dtype(at::kFloat8_e4m3fn);
  auto amax = at::zeros({1}, x.options().dtype(at::kFloat));
  auto q = at::empty({N, F}, q8);
  auto qt = at::empty({F, N}, q8);
  if (N == 0) return {q, qt, amax};
  HIP_OK(launch_bias_gelu_fp8(x.const_data_ptr(), bias.const_data_ptr(),
                              q.data_ptr(), qt.data_ptr(),
                              (const float*)scale.const_data_ptr(),
                              (float*)amax.data_ptr(), N, F, cur_stream()));
  return {q, qt, amax};
}

// h = a (+ delta); LN(h) quantized to e4m3 in both layouts, no bf16 y:
// (h, mean, rstd, q [N, H], qt [H, N], amax [1]), byte-equal to
// add_layer_norm_fwd followed by fp8_quantize(y, scale, dual, e4m3)
std::vector<at::Tensor> add_layer_norm_fp8(
    const at::Tensor& a, const c10::optional<at::Tensor>& b,
    const at::Tensor& w, const at::Tensor& bias, double eps,
    const at::Tensor& scale) {
  auto [N, H] = check_rows(a, "a", 8, a);
  // 16 rows of fp8 bytes are parked in 64 KB of LDS (FLN_MAX_H)
  TORCH_CHECK(H <= 4096, "add_layer_norm_fp8 handles H <= 4096, got ", H);
  TORCH_CHECK(N < kFusedQuantMaxRows, "at most 2^21 rows");
  if (b.has_value()) check_like(*b, "b", a, "a");
  check_vec(w, "w", at::kBFloat16, H, a);
  check_vec(bias, "bias", at::kBFloat16, H, a);
  check_vec(scale, "scale", at::kFloat, 1, a);
  auto f32 = a.options().dtype(at::kFloat);
  auto q8 = a.options().dtype(at::kFloat8_e4m3fn);
  auto h = at::empty_like(a);
  auto mean = at::empty({N}, f32);
  auto rstd = at::empty({N}, f32);
  auto amax = at::zeros({1}, f32);
  auto q = at::empty({N, H}, q8);
  auto qt = at::empty({H, N}, q8);
  if (N == 0) return {h, mean, rstd, q, qt, amax};
  const void* bp = b.has_value() ? b->const_data_ptr() : nullptr;
  HIP_OK(launch_add_layer_norm_fp8(
      a.const_data_ptr(), bp, w.const_data_ptr(), bias.const_data_ptr(),
      h.mutable_data_ptr(), q.data_ptr(), qt.data_ptr(),
      (float*)mean.mutable_data_ptr(), (float*)rstd.mutable_data_ptr(),
      (const float*)scale.const_data_ptr(), (float*)amax.data_ptr(), N, H,
      (float)eps, cur_stream()));
  return {h, mean, rstd, q, qt, amax};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // Bump when the Python<->extension call surface changes; checked by
  // alpa_amd/version.py (reference check_alpa_jaxlib_version, version.py:10)
  // 3: the experimental attention entries (attn_fwd_v2, attn_fwd_sbuf,
  // attn_fwd_ablate, attn_bwd_dkv_ablate) were removed
  // 4: MoE routing entries (moe_route_fwd/bwd, moe_dispatch, moe_combine,
  // moe_combine_dw) added
  // 5: multi_tensor_sumsq_raw added; adamw_step_raw takes grad_sumsq and
  // max_grad_norm
  // 6: bias_gelu_fp8 and add_layer_norm_fp8 added
  // 7: cross_entropy_partial_fwd and cross_entropy_shard_bwd added
  // 8: attn_decode and attn_decode_chunk added
  // 9: layer_norm_bwd, add_layer_norm_bwd, bias_gelu_bwd and colsum_bf16
  // take an optional out_dtype (fp32 or bf16) for the vectors they reduce
  m.attr("ABI_VERSION") = 9;
  m.def("layer_norm_fwd", &layer_norm_fwd, "LayerNorm forward (gfx950)");
  m.def("layer_norm_bwd", &layer_norm_bwd, "LayerNorm backward (gfx950)",
        py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("mean"),
        py::arg("rstd"), py::arg("out_dtype") = py::none());
  m.def("add_layer_norm_fwd", &add_layer_norm_fwd,
        "fused residual-add + LayerNorm fwd (gfx950)");
  m.def("add_layer_norm_bwd", &add_layer_norm_bwd,
        "fused residual-add + LayerNorm bwd (gfx950)", py::arg("dy"),
        py::arg("dh"), py::arg("h"), py::arg("w"), py::arg("mean"),
        py::arg("rstd"), py::arg("out_dtype") = py::none());
  m.def("bias_gelu_fwd", &bias_gelu_fwd, "bias+GeLU forward (gfx950)");
  m.def("bias_gelu_bwd", &bias_gelu_bwd, "bias+GeLU backward (gfx950)",
        py::arg("dy"), py::arg("x"), py::arg("bias"),
        py::arg("out_dtype") = py::none());
  m.def("colsum_bf16", &colsum_bf16, "striped column sum (gfx950)",
        py::arg("t"), py::arg("out_dtype") = py::none());
  m.def("skinny_gemm", &skinny_gemm,
        "decode GEMV over packed weights (gfx950)");
  m.def("adamw_step_raw", &adamw_step_raw, "multi-tensor AdamW (gfx950)",
        py::arg("descs"), py::arg("chunks"), py::arg("step"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("grad_scale"),
        py::arg("grad_sumsq") = py::none(), py::arg("max_grad_norm") = 0.0);
  m.def("multi_tensor_sumsq_raw", &multi_tensor_sumsq_raw,
        "multi-tensor sum of squares (gfx950)");
  m.def("fp8_quantize", &fp8_quantize,
        "one-pass fp8 amax+cast, optional transposed twin (gfx950)");
  m.def("bias_gelu_fp8", &bias_gelu_fp8,
        "bias+GeLU forward emitting e4m3 q, qt and amax (gfx950)");
  m.def("add_layer_norm_fp8", &add_layer_norm_fp8,
        "residual-add + LayerNorm fwd emitting e4m3 q, qt and amax (gfx950)");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused CE fwd (gfx950)");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused CE bwd (gfx950)");
  m.def("cross_entropy_partial_fwd", &cross_entropy_partial_fwd,
        "vocab-shard CE partial stats [3, N] (gfx950)");
  m.def("cross_entropy_shard_bwd", &cross_entropy_shard_bwd,
        "vocab-shard CE bwd (gfx950)");
  m.def("attn_fwd", &attn_fwd, "flash attention fwd (gfx950 MFMA)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"),
        py::arg("scale"), py::arg("alibi") = py::none(),
        py::arg("kv_lens") = py::none());
  m.def("attn_fwd_out", &attn_fwd_out, "flash attention fwd, strided out",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("causal"), py::arg("scale"),
        py::arg("alibi") = py::none(), py::arg("kv_lens") = py::none());
  m.def("attn_decode", &attn_decode,
        "split-KV decode attention, one query row per head (gfx950)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("alibi") = py::none(), py::arg("kv_lens") = py::none());
  m.def("attn_decode_chunk",
        [](int64_t D) { return attn_decode_chunk(D); },
        "keys per split-KV chunk of attn_decode at head_dim D");
  m.def("attn_fwd_blocked", &attn_fwd_blocked,
        "blocked fwd for head_dim > 128 (hipBLASLt scores)");
  m.def("attn_bwd", &attn_bwd, "flash attention bwd (gfx950 MFMA)",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("causal"), py::arg("scale"),
        py::arg("alibi") = py::none());
  m.def("attn_bwd_out", &attn_bwd_out, "flash attention bwd, strided out",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("dq"), py::arg("dk"),
        py::arg("dv"), py::arg("causal"), py::arg("scale"),
        py::arg("alibi") = py::none());
  m.def("attn_bwd_blocked", &attn_bwd_blocked,
        "attention bwd (blocked hipBLASLt reference)");
  m.def("moe_route_fwd", &moe_route_fwd,
        "top-2 gate + capacity slots, sync-free (gfx950)");
  m.def("moe_route_bwd", &moe_route_bwd, "top-2 gate backward (gfx950)");
  m.def("moe_dispatch", &moe_dispatch, "MoE token dispatch gather (gfx950)",
        py::arg("x"), py::arg("src"), py::arg("slot1") = py::none(),
        py::arg("w1") = py::none(), py::arg("w2") = py::none());
  m.def("moe_combine", &moe_combine, "MoE weighted combine gather (gfx950)");
  m.def("moe_combine_dw", &moe_combine_dw,
        "MoE combine gate-weight gradient (gfx950)");
  m.def("mfma_probe", &mfma_probe, "MFMA 16x16x32 layout probe");
  m.def("mfma_probe32", &mfma_probe32, "MFMA 32x32x16 layout probe");
}
