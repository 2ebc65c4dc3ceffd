"""Hot-op library: hand-written CDNA4 (gfx950) HIP kernels with autograd.

Dispatch: CUDA(ROCm) tensors -> the in-tree HIP extension (`_hip_ops.so`,
built from ``csrc/``); CPU tensors -> the pure-torch reference
(`reference.py`).  Plain unfused GEMMs go through ``torch.matmul``
(hipBLASLt on ROCm) — hand-written kernels cover the *fused* ops where
library calls can't: LayerNorm, flash attention, bias+GeLU epilogue,
softmax-cross-entropy over the 51200-wide vocab and over its tensor-parallel
shards (softmax_cross_entropy_partial / _combine / _shard_bwd: per-shard
row statistics, one [N]-sized combine, a collective-free backward),
multi-tensor AdamW with global-norm gradient clipping (multi_tensor_sumsq
feeds fused_adamw), and the sync-free top-2 MoE routing path: moe_top2_route (gate + capacity
slots), moe_dispatch and moe_combine.  add_layer_norm_fp8 and bias_gelu_fp8
are the LayerNorm and GeLU forwards with the fp8 quantize of ops/fp8.py
folded in.  flash_attention_decode is the split-KV attention kernel for
single-token queries, which flash_attention and flash_attention_varlen use
for every decode step.  kv_cache_append_fp8 and flash_attention_decode_fp8
are the write and the read side of the e4m3 KV cache (one fp32 scale per
cached row), which global_config.kv_cache_fp8 turns on in the decoders.
flash_attention_chunk and flash_attention_chunk_fp8 are the split-KV MFMA
kernel for several query rows over a cache that already holds them (chunked
prefill, draft verification, a multi-token turn), causal at the end of the
cache.  qkv_cache_write is what runs between the qkv projection and those
attention kernels in a cached decoder step, as one kernel: it splits the
packed projection, applies the rotary transform to q and k (CodeGen), writes
q contiguous and writes k and v into the bf16 or e4m3 cache at per-slot
positions read on the device (global_config.fused_qkv_write;
qkv_cache_write_ok is its envelope).  skinny_ok / skinny_linear are the
packed decode GEMMs for up to 64
tokens (dot2 GEMV up to 8, MFMA skinny GEMM for 9..64) over bf16, e4m3 or,
under global_config.weight_fp4, MXFP4 weights: mxfp4_quantize and
mxfp4_dequantize are that format (e2m1 codes, one e8m0 scale per 32 k),
mxfp4_pack the layout its two kernels read.  weight_twin and its helpers
keep the transposed copies of linear weights that fused_adamw writes and
linear_bias's dX GEMM reads.  logits_topk and sample_logits are the pass over
the vocabulary that ends a decode step (top-k with the softmax max and
sum-exp in one read of the row; temperature / top-k / top-p sampling with
per-row parameters read on the device), which global_config.fused_sampling
turns on in generation, beam search and the batcher; logits_topk_ok is
their envelope.

Kernel-level contract mirrors the reference's compiled-HLO op inventory
(GEMM+epilogue, attention, LayerNorm, fused Adam,
grad accumulation, collectives).
"""
from __future__ import annotations

import functools
import math
import weakref
from typing import List, NamedTuple, Optional

import torch

from . import reference as ref
from ._backend import hip_ops, hip_ops_available, use_hip

__all__ = [
    "layer_norm", "add_layer_norm", "bias_gelu", "add_layer_norm_fp8",
    "bias_gelu_fp8", "flash_attention",
    "flash_attention_qkv", "flash_attention_decode", "decode_attn_ok",
    "DECODE_ATTN_CHUNK", "kv_cache_append_fp8", "qkv_cache_write",
    "qkv_cache_write_ok",
    "flash_attention_decode_fp8", "decode_attn_fp8_ok",
    "flash_attention_chunk", "chunk_attn_ok", "flash_attention_chunk_fp8",
    "chunk_attn_fp8_ok",
    "softmax_cross_entropy",
    "softmax_cross_entropy_partial", "softmax_cross_entropy_combine",
    "softmax_cross_entropy_shard_bwd", "vocab_ce_fused_ok",
    "logits_topk", "logits_topk_ok", "sample_logits", "LOGITS_TOPK_SEG",
    "fused_adamw",
    "multi_tensor_sumsq", "weight_twin", "weight_twin_eligible",
    "register_weight_twin", "weight_twin_written", "valid_weight_twin",
    "invalidate_weight_twin",
    "hip_ops_available", "MoERouting", "moe_top2_route", "moe_dispatch",
    "moe_combine", "moe_fused_ok",
    "skinny_ok", "skinny_linear", "mxfp4_quantize", "mxfp4_dequantize",
    "mxfp4_pack",
]


class _LayerNorm(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        if use_hip(x):
            y, mean, rstd = hip_ops().layer_norm_fwd(x, weight, bias, eps)
        else:
            y, mean, rstd = ref.layer_norm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        if use_hip(x):
            # dw and db leave the extension in the parameter dtype
            dx, dw, db = hip_ops().layer_norm_bwd(dy.contiguous(), x, weight,
                                                  mean, rstd, weight.dtype)
        else:
            dx, dw, db = ref.layer_norm_bwd(dy, x, weight, mean, rstd)
            dw, db = dw.to(weight.dtype), db.to(weight.dtype)
        return dx, dw, db, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    return _LayerNorm.apply(x, weight, bias, eps)


class _AddLayerNorm(torch.autograd.Function):
    """Fused h = a + delta; y = LN(h).  Returns (h, y) — h feeds the
    residual stream, y the block input.  Saves the separate residual-add
    HBM pass (XLA fusion analog)."""

    @staticmethod
    def forward(ctx, a, delta, weight, bias, eps):
        a = a.contiguous()
        delta = delta.contiguous() if delta is not None else None
        if use_hip(a):
            h, y, mean, rstd = hip_ops().add_layer_norm_fwd(
                a, delta, weight, bias, eps)
        else:
            h = a + delta if delta is not None else a
            y, mean, rstd = ref.layer_norm_fwd(h, weight, bias, eps)
        ctx.save_for_backward(h, weight, mean, rstd)
        ctx.has_delta = delta is not None
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, weight, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dhc = dh.contiguous() if dh is not None else None
        if use_hip(h):
            dx, dw, db = hip_ops().add_layer_norm_bwd(
                dy, dhc, h, weight, mean, rstd, weight.dtype)
        else:
            dx, dw, db = ref.layer_norm_bwd(dy, h, weight, mean, rstd)
            dw, db = dw.to(weight.dtype), db.to(weight.dtype)
            if dhc is not None:
                dx = dx + dhc
        g2 = dx if ctx.has_delta else None
        return dx, g2, dw, db, None


def add_layer_norm(a: torch.Tensor, delta, weight: torch.Tensor,
                   bias: torch.Tensor, eps: float = 1e-5):
    """(h, y) = (a [+ delta], LN(a [+ delta])).  delta may be None."""
    if delta is None:
        # no add to fuse: plain LN, h aliases a
        return a, _LayerNorm.apply(a, weight, bias, eps)
    return _AddLayerNorm.apply(a, delta, weight, bias, eps)


class _BiasGelu(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, bias):
        x = x.contiguous()
        ctx.save_for_backward(x, bias)
        if use_hip(x):
            return hip_ops().bias_gelu_fwd(x, bias)
        return ref.bias_gelu_fwd(x, bias)

    @staticmethod
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        if use_hip(x):
            dx, db = hip_ops().bias_gelu_bwd(dy.contiguous(), x, bias,
                                             bias.dtype)
        else:
            dx, db = ref.bias_gelu_bwd(dy, x, bias)
            db = db.to(bias.dtype)
        return dx, db


def bias_gelu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Fused (x + bias) -> gelu_tanh. The epilogue of the MLP up-projection."""
    return _BiasGelu.apply(x, bias)


@torch.no_grad()
def bias_gelu_fp8(x: torch.Tensor, bias: torch.Tensor, scale: torch.Tensor):
    """gelu(x + bias) quantized straight to e4m3 for an fp8 GEMM, without
    writing the bf16 activation: (q [N, F], qt [F, N], amax fp32 [1]) for
    x [.., F], N = x.numel() / F.  `scale` is the delayed per-tensor scale
    (fp32 [1] on x's device), amax the largest |gelu(x + bias)| after
    rounding to bf16.  On the GPU the result is byte-for-byte that of
    bias_gelu followed by the dual-layout quantize kernel.  Forward only:
    ops.fp8.fp8_gelu_linear is the autograd user."""
    x = x.contiguous()
    if use_hip(x):
        return tuple(hip_ops().bias_gelu_fp8(x, bias, scale))
    return ref.bias_gelu_fp8(x, bias, scale)


#: widest row ops.add_layer_norm_fp8 takes on the GPU: its kernel parks 16
#: rows of fp8 bytes in 64 KB of LDS (FLN_MAX_H in csrc/fp8_fused.hip)
ADD_LAYER_NORM_FP8_MAX_H = 4096


@torch.no_grad()
def add_layer_norm_fp8(a: torch.Tensor, delta, weight: torch.Tensor,
                       bias: torch.Tensor, eps: float, scale: torch.Tensor):
    """h = a (+ delta); LN(h) quantized straight to e4m3 for an fp8 GEMM,
    without writing the bf16 normalized tensor: (h, mean [N], rstd [N],
    q [N, H], qt [H, N], amax fp32 [1]).  delta may be None (h is then a
    copy of a).  On the GPU the result is byte-for-byte that of
    add_layer_norm followed by the dual-layout quantize kernel, and H is
    at most ADD_LAYER_NORM_FP8_MAX_H.  Forward only: ops.fp8.fp8_ln_linear
    is the autograd user."""
    a = a.contiguous()
    delta = delta.contiguous() if delta is not None else None
    if use_hip(a):
        return tuple(hip_ops().add_layer_norm_fp8(a, delta, weight, bias,
                                                  eps, scale))
    return ref.add_layer_norm_fp8(a, delta, weight, bias, eps, scale)


def _colsum(g2: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Column sum of bf16 rows [N, F] on the striped HIP kernels, reduced on
    the device straight into `dtype` (a bias's)."""
    if dtype in (torch.bfloat16, torch.float32):
        return hip_ops().colsum_bf16(g2, dtype)
    return hip_ops().colsum_bf16(g2).to(dtype)


class _BiasAdd(torch.autograd.Function):
    """y = x + bias with the bias-grad column sum on the striped HIP
    kernel (torch's reduce path for broadcast-add backward cost ~8 ms
    per GPT-2.6B step in the r2 profile)."""

    @staticmethod
    def forward(ctx, x, bias):
        ctx.feat = bias.shape[-1]
        ctx.bias_dtype = bias.dtype
        return x + bias

    @staticmethod
    def backward(ctx, g):
        if use_hip(g) and g.dtype == torch.bfloat16:
            db = _colsum(g.contiguous().reshape(-1, ctx.feat),
                         ctx.bias_dtype)
        else:
            dims = tuple(range(g.dim() - 1))
            db = g.sum(dim=dims).to(ctx.bias_dtype)
        return g, db


def bias_add(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Broadcast bias add whose backward reduces on the HIP column-sum
    (drop-in for `x + bias` on [.., F] activations)."""
    return _BiasAdd.apply(x, bias)


class _LinearBias(torch.autograd.Function):
    """y = x @ w.T (+ bias).  With a bias, via torch.addmm: hipBLASLt fuses
    the bias epilogue into the GEMM (measured free — matmul+separate add
    cost ~16 ms per GPT-2.6B step, tools/addmm_probe.py).  Backward runs
    the standard dX/dW GEMMs and the HIP column-sum for db; dX reads the
    weight's twin (valid_weight_twin) where it has one, which turns the NN
    GEMM dY @ w into the TN form dY @ twin.t() of the same product."""

    @staticmethod
    def forward(ctx, x, w, bias):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if bias is None:
            y = torch.matmul(x2, w.t())
        else:
            y = torch.addmm(bias, x2, w.t())
            ctx.bias_dtype = bias.dtype
        ctx.save_for_backward(x2, w)
        ctx.has_bias = bias is not None
        return y.reshape(*shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x2, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        twin = valid_weight_twin(w)
        dx = (g2 @ w) if twin is None else (g2 @ twin.t())
        dx = dx.reshape(*g.shape[:-1], w.shape[1])
        dw = g2.t() @ x2
        if not ctx.has_bias:
            return dx, dw, None
        if use_hip(g2) and g2.dtype == torch.bfloat16:
            db = _colsum(g2, ctx.bias_dtype)
        else:
            db = g2.sum(0).to(ctx.bias_dtype)
        return dx, dw, db


def linear_bias(x: torch.Tensor, w: torch.Tensor,
                bias: Optional[torch.Tensor]) -> torch.Tensor:
    """F.linear with the bias (if any) fused into the hipBLASLt epilogue,
    the bias grad on the HIP column-sum and dX on the weight's twin."""
    return _LinearBias.apply(x, w, bias)


class _FlashAttention(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, alibi=None):
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        if use_hip(q):
            if q.shape[-1] > 128:
                # big heads (CodeGen-6B/16B: 256): the fused Dp=256
                # instantiation (single-buffered K/V, 512 threads) runs
                # PREFILL 3.3-5x faster than the blocked hipBLASLt path
                # (241 vs 70 TF at S=2048, tools/d256_probe.py); the
                # blocked path keeps the few-row calls that reach this
                # function (single-token decode goes to the split-KV
                # kernel in flash_attention unless autograd records it or
                # decode_attention is "0").  No alibi at D>128 (BLOOM
                # heads are <=128).
                assert alibi is None, "alibi requires head_dim <= 128"
                if q.shape[2] >= 128 and q.shape[-1] <= 256:
                    o, lse = hip_ops().attn_fwd(q, k, v, causal, scale,
                                                None)
                else:
                    o, lse = hip_ops().attn_fwd_blocked(q, k, v, causal,
                                                        scale)
            else:
                o, lse = hip_ops().attn_fwd(q, k, v, causal, scale, alibi)
        else:
            o, lse = ref.attention_fwd(q, k, v, causal, scale, alibi)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.scale = scale
        ctx.alibi = alibi
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        if use_hip(q):
            if q.shape[-1] > 128:
                dq, dk, dv = hip_ops().attn_bwd_blocked(
                    do.contiguous(), q, k, v, o, lse, ctx.causal, ctx.scale)
            else:
                dq, dk, dv = hip_ops().attn_bwd(
                    do.contiguous(), q, k, v, o, lse, ctx.causal, ctx.scale,
                    ctx.alibi)
        else:
            dq, dk, dv = ref.attention_bwd(do, q, k, v, o, lse, ctx.causal,
                                           ctx.scale, ctx.alibi)
        return dq, dk, dv, None, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = True,
                    scale: Optional[float] = None,
                    alibi_slopes: Optional[torch.Tensor] = None
                    ) -> torch.Tensor:
    """Fused attention. q,k,v: [B, heads, S, head_dim] (bf16 on GPU).

    Online-softmax tiling — never materializes the S x S score matrix
    (reference's compiled modules get this from XLA fusion; here it is the
    hand-written gfx950 kernel).  alibi_slopes [heads]
    (fp32) adds the BLOOM ALiBi bias inside the kernel.
    """
    if q.shape[2] == 1 and not causal and _decode_attn_routed(q, k, v) and \
            not (torch.is_grad_enabled() and
                 (q.requires_grad or k.requires_grad or v.requires_grad)):
        # single-token decode outside autograd: the split-KV kernel
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        return hip_ops().attn_decode(q, k, v, scale, alibi_slopes, None)[0]
    return _FlashAttention.apply(q, k, v, causal, scale, alibi_slopes)


# keys per split-KV chunk by padded head dim; must match DecodeChunk in
# csrc/attention_decode.hip (the extension's attn_decode_chunk reports it)
_DECODE_ATTN_CHUNK = {64: 128, 128: 128, 256: 128}


def DECODE_ATTN_CHUNK(head_dim: int) -> int:
    """Keys per chunk of the split-KV decode kernel at this head_dim.  A
    function of head_dim alone — never of the batch, the heads, the cache
    length or the device — which is what makes a slot's output bits
    independent of its neighbours and of the cache capacity."""
    for dp in sorted(_DECODE_ATTN_CHUNK):
        if head_dim <= dp:
            return _DECODE_ATTN_CHUNK[dp]
    raise ValueError(f"head_dim {head_dim} is above 256")


def _rows_aligned16(t: torch.Tensor) -> bool:
    return t.data_ptr() % 16 == 0 and all(
        t.shape[i] <= 1 or t.stride(i) % 8 == 0 for i in range(3))


def chunk_attn_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Envelope of the split-KV kernels over a bf16 cache
    (csrc/attention_chunk.hip, and with one query row
    csrc/attention_decode.hip; the bindings check the same): bf16 on the
    GPU, q [B, h, Sq, d] and k, v [B, h, Skv, d] views with a contiguous
    head dim, d a multiple of 16 up to 256, and every row 16-byte aligned
    (aligned base, batch/head/seq strides multiples of 8 elements) for the
    16-byte loads.  Sq is free: flash_attention_chunk cuts it into launches
    of at most 64 rows."""
    for t in (q, k, v):
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
                and t.stride(3) == 1):
            return False
    D = q.shape[3]
    if q.shape[2] < 1 or D % 16 != 0 or not 16 <= D <= 256:
        return False
    if k.shape != v.shape or k.shape[:2] != q.shape[:2] or k.shape[3] != D \
            or q.shape[0] * q.shape[1] > 65535:
        return False
    if not all(_rows_aligned16(t) for t in (q, k, v)):
        return False
    return use_hip(q)


def decode_attn_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Envelope of the split-KV decode attention kernel
    (csrc/attention_decode.hip): chunk_attn_ok with exactly one query row,
    q [B, h, 1, d]."""
    return q.dim() == 4 and q.shape[2] == 1 and chunk_attn_ok(q, k, v)


def _decode_attn_routed(q, k, v) -> bool:
    """Do flash_attention / flash_attention_varlen send this single-token
    call to the split-KV kernel?  global_config.decode_attention: "0" never,
    "1" and "auto" whenever the call is inside the envelope (the rule and
    its evidence are on the config field)."""
    from ..global_env import global_config
    if global_config.decode_attention in ("0", False):
        return False
    return decode_attn_ok(q, k, v)


@torch.no_grad()
def flash_attention_decode(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           kv_lens: Optional[torch.Tensor] = None,
                           scale: Optional[float] = None,
                           alibi_slopes: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
    """Single-token decode attention: q [B, h, 1, d] attends, unmasked, to
    the first kv_lens[b] (default all Skv) rows of k, v [B, h, Skv, d];
    returns o [B, h, 1, d].  Inference only.

    Inside decode_attn_ok this is the split-KV gfx950 kernel: the cache is
    cut into chunks of DECODE_ATTN_CHUNK(d) keys, one workgroup each, and a
    second launch merges them.  It reads strided views (a cache slice, the
    q of a packed qkv projection) in place, never loads a row at or past a
    slot's length, keeps P in fp32, and a slot's output bits depend only on
    that slot's own q, visible k/v rows, length, d, scale and slope.  A slot
    of length 0 gives o = 0.  kv_lens may live on the device, so the call
    can be captured in a graph.  On CPU or outside the envelope it is
    reference.attention_fwd."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    lens = None if kv_lens is None else kv_lens.to(dtype=torch.int32)
    if decode_attn_ok(q, k, v):
        return hip_ops().attn_decode(
            q, k, v, scale, alibi_slopes,
            None if lens is None else lens.contiguous())[0]
    o, _ = ref.attention_fwd(q, k, v, False, scale, alibi_slopes, lens)
    return o


def _kv8_ok(c8: torch.Tensor, cs: torch.Tensor, first: torch.Tensor,
            align: int) -> bool:
    """One half of an e4m3 cache: bytes [B, h, L, d] float8_e4m3fn with a
    contiguous head dim and rows aligned to `align` bytes, and its scales
    [B, h, L] fp32, both on the device of `first`."""
    if not (c8.is_cuda and c8.device == first.device
            and c8.dtype == torch.float8_e4m3fn and c8.dim() == 4
            and c8.stride(3) == 1):
        return False
    if c8.data_ptr() % align != 0 or not all(
            c8.shape[i] <= 1 or c8.stride(i) % align == 0 for i in range(3)):
        return False
    return (cs.is_cuda and cs.device == first.device
            and cs.dtype == torch.float32 and cs.shape == c8.shape[:3])


def chunk_attn_fp8_ok(q: torch.Tensor, k8: torch.Tensor,
                      k_scale: torch.Tensor, v8: torch.Tensor,
                      v_scale: torch.Tensor) -> bool:
    """Envelope of the split-KV kernels over an e4m3 cache
    (csrc/attention_chunk.hip, and with one query row
    csrc/attention_decode_fp8.hip; the bindings check the same).  It is
    chunk_attn_ok with the cache in bytes: q bf16 [B, h, Sq, d] on the GPU,
    k8, v8 [B, h, Skv, d] float8_e4m3fn views with a contiguous head dim, d
    a multiple of 16 up to 256, every q row and every cache row 16-byte
    aligned; plus k_scale, v_scale fp32 [B, h, Skv] on the same device (any
    strides)."""
    if not (q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 4
            and q.stride(3) == 1 and _rows_aligned16(q)):
        return False
    D = q.shape[3]
    if q.shape[2] < 1 or D % 16 != 0 or not 16 <= D <= 256 \
            or q.shape[0] * q.shape[1] > 65535:
        return False
    if not (_kv8_ok(k8, k_scale, q, 16) and _kv8_ok(v8, v_scale, q, 16)):
        return False
    if k8.shape != v8.shape or k8.shape[:2] != q.shape[:2] \
            or k8.shape[3] != D:
        return False
    return use_hip(q)


def decode_attn_fp8_ok(q: torch.Tensor, k8: torch.Tensor,
                       k_scale: torch.Tensor, v8: torch.Tensor,
                       v_scale: torch.Tensor) -> bool:
    """Envelope of the e4m3-cache decode kernel
    (csrc/attention_decode_fp8.hip): chunk_attn_fp8_ok with exactly one
    query row, q [B, h, 1, d]."""
    return q.dim() == 4 and q.shape[2] == 1 and \
        chunk_attn_fp8_ok(q, k8, k_scale, v8, v_scale)


def _kv_append_ok(k, v, k8, k_scale, v8, v_scale, pos) -> bool:
    """Envelope of csrc/kv_cache_fp8.hip: k, v bf16 [B, h, S, d] views on
    the GPU with a contiguous head dim and 16-byte-aligned rows, d a multiple
    of 16 in [16, 256], cache rows 8-byte aligned, pos an int or a contiguous
    int32/int64 [B] on the device."""
    for t in (k, v):
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
                and t.stride(3) == 1 and _rows_aligned16(t)):
            return False
    D = k.shape[3]
    if k.shape != v.shape or D % 16 != 0 or not 16 <= D <= 256:
        return False
    if not (_kv8_ok(k8, k_scale, k, 8) and _kv8_ok(v8, v_scale, k, 8)):
        return False
    if k8.shape != v8.shape or k8.shape[:2] != k.shape[:2] \
            or k8.shape[3] != D:
        return False
    if torch.is_tensor(pos) and not (
            pos.device == k.device and pos.is_contiguous()
            and pos.dtype in (torch.int32, torch.int64)
            and pos.shape == (k.shape[0],)):
        return False
    return use_hip(k)


@torch.no_grad()
def kv_cache_append_fp8(k: torch.Tensor, v: torch.Tensor, k8: torch.Tensor,
                        k_scale: torch.Tensor, v8: torch.Tensor,
                        v_scale: torch.Tensor, pos) -> None:
    """Quantize the new rows k, v [B, h, S, d] to e4m3 and write them into
    the cache k8, v8 [B, h, max_len, d] (float8_e4m3fn) with k_scale, v_scale
    [B, h, max_len] (fp32), in place: row (b, h, s) goes to position
    pos_b + s, where pos is one int or an int tensor [B].

    Every row carries its own scale: scale = amax(|x|) / 448 and bytes =
    e4m3_rne(x / scale), both in fp32, saturating.  An all-zero row stores
    scale = 1.  A row that holds a NaN or an Inf stores scale = NaN and the
    byte 0x7F throughout, so it dequantizes to NaN and poisons the slot that
    attends to it instead of being clamped.  A row whose position is
    negative or >= max_len is skipped.  Older rows are never touched.

    On the GPU this is one launch of the gfx950 kernel for K and V together;
    it reads strided views (the k and v of a packed qkv projection) in place
    and takes pos from the device without a host read, so it can be captured
    in a graph.  On CPU or outside the kernel's envelope it is
    reference.kv_cache_append_fp8."""
    if _kv_append_ok(k, v, k8, k_scale, v8, v_scale, pos):
        if torch.is_tensor(pos):
            hip_ops().kv_cache_append(k, v, k8, k_scale, v8, v_scale, 0, pos)
        else:
            hip_ops().kv_cache_append(k, v, k8, k_scale, v8, v_scale,
                                      int(pos), None)
        return
    ref.kv_cache_append_fp8(k, v, k8, k_scale, v8, v_scale, pos)


def qkv_cache_write_ok(qkv: torch.Tensor, cache_k, cache_v, pos,
                       rotary) -> bool:
    """Envelope of csrc/qkv_cache_write.hip (the binding checks the same):
    qkv a bf16 [B, S, h, 3, d] view on the GPU with stride(4) == 1,
    stride(3) == d, B/S/h strides that are multiples of 8 elements and a
    16-byte-aligned base, d a multiple of 16 in [16, 256]; cache_k and cache_v
    what KVCache.layer returns: bf16 [B, h, L, d] views with a contiguous head
    dim and 16-byte-aligned rows, or (bytes, scales) pairs inside
    _kv8_ok(.., 8); pos an int or a contiguous int32/int64 [B] on the device;
    rotary None or (sin, cos, rotary_dim) with contiguous 16-byte-aligned
    [T, rotary_dim/2] tables of one dtype, fp32 or bf16, on the device,
    rotary_dim a multiple of 8 in (0, d]."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda
            and qkv.dtype == torch.bfloat16 and qkv.dim() == 5
            and qkv.shape[3] == 3 and qkv.stride(4) == 1
            and qkv.stride(3) == qkv.shape[4] and _rows_aligned16(qkv)):
        return False
    B, S, h, _, D = qkv.shape
    if D % 16 != 0 or not 16 <= D <= 256 or B * S * h >= 2 ** 31:
        return False
    if isinstance(cache_k, tuple) != isinstance(cache_v, tuple):
        return False
    if isinstance(cache_k, tuple):
        (ck, ks), (cv, vs) = cache_k, cache_v
        if not (_kv8_ok(ck, ks, qkv, 8) and _kv8_ok(cv, vs, qkv, 8)):
            return False
    else:
        ck, cv = cache_k, cache_v
        for t in (ck, cv):
            if not (t.is_cuda and t.device == qkv.device
                    and t.dtype == torch.bfloat16 and t.dim() == 4
                    and t.stride(3) == 1 and _rows_aligned16(t)):
                return False
    if ck.shape != cv.shape or ck.shape[:2] != (B, h) or ck.shape[3] != D:
        return False
    if torch.is_tensor(pos) and not (
            pos.device == qkv.device and pos.is_contiguous()
            and pos.dtype in (torch.int32, torch.int64)
            and pos.shape == (B,)):
        return False
    if rotary is not None:
        sin, cos, rd = rotary
        if rd % 8 != 0 or not 0 < rd <= D:
            return False
        for t in (sin, cos):
            if not (t.is_cuda and t.device == qkv.device
                    and t.dtype == sin.dtype
                    and t.dtype in (torch.float32, torch.bfloat16)
                    and t.dim() == 2 and t.shape == (sin.shape[0], rd // 2)
                    and t.is_contiguous() and t.data_ptr() % 16 == 0):
                return False
    return use_hip(qkv)


@torch.no_grad()
def qkv_cache_write(qkv: torch.Tensor, cache_k, cache_v, pos, rotary=None,
                    want_k: bool = False, _in_envelope: bool = False):
    """Everything between the qkv projection and the attention kernel of a
    cached decoder step: split the packed qkv [B, S, h, 3, d], rotate q and
    k, and write k and v into the KV cache.  Returns q [B, h, S, d]
    contiguous, or (q, k_new) with want_k (k_new the rotated k, same shape).
    Inference only.

    cache_k and cache_v are what KVCache.layer returns, views included: bf16
    [B, h, L, d], or (bytes, scales) pairs of the e4m3 cache.  Row
    (b, head, s) sits at position p = pos_b + s and goes to cache row p; pos
    is an int or an int32/int64 [B] tensor, read on the device only, so the
    call can be captured in a graph.  rotary is None or (sin, cos,
    rotary_dim) with tables [T, rotary_dim/2], fp32 or bf16: GPT-J interleaved
    pairs on the first rotary_dim columns, y0 = x0*c - x1*s and y1 = x0*s +
    x1*c in fp32 with every operation rounded on its own, then rounded to
    bf16 once.  The other columns and v are copied bit for bit; an e4m3 cache
    row is what kv_cache_append_fp8 makes of the rounded row.  A row with p
    outside [0, L), or outside the tables, is zero in q (and k_new) and
    writes nothing to the cache; an int pos whose rows leave the tables is
    refused.  Older cache rows are never touched.

    Inside qkv_cache_write_ok this is one launch of the gfx950 kernel
    (csrc/qkv_cache_write.hip), which reads qkv in place.  On CPU or outside
    the envelope it is reference.qkv_cache_write.  (_in_envelope: the caller
    has just had True from qkv_cache_write_ok for these operands, so the
    Python-side check is not repeated; the binding checks them in any case.)"""
    if not (_in_envelope or
            qkv_cache_write_ok(qkv, cache_k, cache_v, pos, rotary)):
        return ref.qkv_cache_write(qkv, cache_k, cache_v, pos, rotary, want_k)
    if isinstance(cache_k, tuple):
        (ck, ks), (cv, vs) = cache_k, cache_v
    else:
        ck, cv, ks, vs = cache_k, cache_v, None, None
    sin, cos, rd = rotary if rotary is not None else (None, None, 0)
    host, dev = (0, pos) if torch.is_tensor(pos) else (int(pos), None)
    out = hip_ops().qkv_cache_write(qkv, ck, cv, ks, vs, host, dev, sin, cos,
                                    rd, want_k)
    return tuple(out) if want_k else out[0]


@torch.no_grad()
def flash_attention_decode_fp8(q: torch.Tensor, k8: torch.Tensor,
                               k_scale: torch.Tensor, v8: torch.Tensor,
                               v_scale: torch.Tensor,
                               kv_lens: Optional[torch.Tensor] = None,
                               scale: Optional[float] = None,
                               alibi_slopes: Optional[torch.Tensor] = None
                               ) -> torch.Tensor:
    """flash_attention_decode over the e4m3 cache that kv_cache_append_fp8
    writes: q [B, h, 1, d] attends to the first kv_lens[b] (default all Skv)
    rows of k8, v8 [B, h, Skv, d] with per-row scales [B, h, Skv]; returns
    o [B, h, 1, d] in q's dtype.  Inference only.

    Inside decode_attn_fp8_ok this is the split-KV gfx950 kernel with the
    chunking of the bf16 one (DECODE_ATTN_CHUNK); it streams half the bytes.
    All math is fp32: s = (q . k8_row) * k_scale[row] * scale, P is not
    rounded, v_scale[row] is folded into p.  Rows at or past a slot's length
    are never loaded, scales included, and a slot's output bits depend only
    on that slot's own q, visible rows and scales, length, d, scale and
    slope.  A slot of length 0 gives o = 0; a visible row with a NaN scale
    gives a NaN output.  On CPU or outside the envelope it is
    reference.attention_decode_fp8."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    lens = None if kv_lens is None else kv_lens.to(dtype=torch.int32)
    if decode_attn_fp8_ok(q, k8, k_scale, v8, v_scale):
        return hip_ops().attn_decode_fp8(
            q, k8, k_scale, v8, v_scale, scale, alibi_slopes,
            None if lens is None else lens.contiguous())[0]
    o, _ = ref.attention_decode_fp8(q, k8, k_scale, v8, v_scale, scale,
                                    alibi_slopes, lens)
    return o


# query rows per launch of csrc/attention_chunk.hip (its QT = 4 instantiation)
_CHUNK_ATTN_MAX_ROWS = 64


def _chunk_pieces(Sq: int, Skv: int, lens: Optional[torch.Tensor]):
    """Cut Sq query rows into launches of at most 64: piece [a, b) sits
    Sq - b rows before the end of its slot, so it runs with the slot's
    length less Sq - b.  Yields (a, b, cache rows to pass, lengths): with
    lengths they are computed on the device and the whole view is passed;
    without, the view is cut instead.  No host read either way."""
    for a in range(0, Sq, _CHUNK_ATTN_MAX_ROWS):
        b = min(a + _CHUNK_ATTN_MAX_ROWS, Sq)
        if lens is None:
            yield a, b, max(Skv - (Sq - b), 0), None
        else:
            yield a, b, Skv, (lens if b == Sq else lens - (Sq - b))


@torch.no_grad()
def flash_attention_chunk(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                          kv_lens: Optional[torch.Tensor] = None,
                          scale: Optional[float] = None,
                          alibi_slopes: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """Attention of Sq new query rows over a cache that already holds them:
    q [B, h, Sq, d]; k, v [B, h, Skv, d], of which slot b uses the first
    len_b = kv_lens[b] (default Skv) rows, the last Sq of them being the new
    ones.  Query row i sits at position len_b - Sq + i and sees keys up to
    and including that position (a causal mask aligned with the end of the
    cache); a row at a negative position gives o = 0.  Returns o
    [B, h, Sq, d].  Inference only; any Sq >= 1.

    Inside chunk_attn_ok this is the split-KV MFMA kernel for gfx950
    (csrc/attention_chunk.hip): one workgroup per DECODE_ATTN_CHUNK(d) keys
    takes up to 64 query rows through QK^T, a one-tile softmax and PV on
    matrix instructions, and a second launch merges the chunks; longer q
    runs as pieces of at most 64 rows.  It reads strided views in place,
    never loads a row at or past a slot's length, rounds P to bf16 once, and
    a slot's output bits depend only on that slot's own q, visible k/v
    rows, length, Sq, d, scale and slope.  kv_lens may live on the device:
    there is no host read, so the call can be captured in a graph.  On CPU
    or outside the envelope it is reference.attention_chunk."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    lens = None if kv_lens is None else kv_lens.to(dtype=torch.int32)
    if not chunk_attn_ok(q, k, v):
        return ref.attention_chunk(q, k, v, scale, alibi_slopes, lens)[0]
    Sq, Skv = q.shape[2], k.shape[2]
    outs = [hip_ops().attn_chunk(
        q[:, :, a:b], k[:, :, :n], v[:, :, :n], scale, alibi_slopes,
        None if ln is None else ln.contiguous())[0]
        for a, b, n, ln in _chunk_pieces(Sq, Skv, lens)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)


@torch.no_grad()
def flash_attention_chunk_fp8(q: torch.Tensor, k8: torch.Tensor,
                              k_scale: torch.Tensor, v8: torch.Tensor,
                              v_scale: torch.Tensor,
                              kv_lens: Optional[torch.Tensor] = None,
                              scale: Optional[float] = None,
                              alibi_slopes: Optional[torch.Tensor] = None
                              ) -> torch.Tensor:
    """flash_attention_chunk over the e4m3 cache that kv_cache_append_fp8
    writes: k8, v8 [B, h, Skv, d] with per-row scales [B, h, Skv]; returns
    o [B, h, Sq, d] in q's dtype.  Inference only.

    Inside chunk_attn_fp8_ok this is the e4m3 instantiation of the same
    kernel: K bytes become bf16 in registers and k_scale[row] multiplies the
    fp32 score; V bytes become bf16 while they are staged and v_scale[row]
    is folded into p in fp32 before its one rounding to bf16.  Rows at or
    past a slot's length are never loaded, scales included; a visible row
    with a NaN scale gives a NaN output.  On CPU or outside the envelope it
    is reference.attention_chunk_fp8."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    lens = None if kv_lens is None else kv_lens.to(dtype=torch.int32)
    if not chunk_attn_fp8_ok(q, k8, k_scale, v8, v_scale):
        return ref.attention_chunk_fp8(q, k8, k_scale, v8, v_scale, scale,
                                       alibi_slopes, lens)[0]
    Sq, Skv = q.shape[2], k8.shape[2]
    outs = [hip_ops().attn_chunk_fp8(
        q[:, :, a:b], k8[:, :, :n], k_scale[:, :, :n], v8[:, :, :n],
        v_scale[:, :, :n], scale, alibi_slopes,
        None if ln is None else ln.contiguous())[0]
        for a, b, n, ln in _chunk_pieces(Sq, Skv, lens)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)


@torch.no_grad()
def flash_attention_varlen(q: torch.Tensor, k: torch.Tensor,
                           v: torch.Tensor, kv_lens: torch.Tensor,
                           scale: Optional[float] = None,
                           alibi_slopes: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
    """Decode attention with PER-BATCH KV lengths (continuous batching):
    slot b's queries attend to k[b, :, :kv_lens[b]].  Inference-only
    (no backward); the gfx950 kernel masks per element past each slot's
    length and never loads k or v there, so a stale NaN or Inf in a cache
    tail is harmless.  A slot of length 0 gives o = 0.  Single-token
    queries go to the split-KV decode kernel (flash_attention_decode),
    which also takes head_dim up to 256 and reads the cache view in
    place."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    lens = kv_lens.to(dtype=torch.int32)
    if use_hip(q):
        if q.shape[2] == 1 and _decode_attn_routed(q, k, v):
            return hip_ops().attn_decode(q, k, v, scale, alibi_slopes,
                                         lens.contiguous())[0]
        if q.shape[-1] > 128:
            # the prefill kernel's varlen template is instantiated for
            # head_dim <= 128: wider heads have the single-token decode
            # kernel above only
            raise NotImplementedError(
                "varlen attention with more than one query row, or with "
                "the decode kernel off, requires head_dim <= 128")
        o, _ = hip_ops().attn_fwd(q.contiguous(), k.contiguous(),
                                  v.contiguous(), False, scale,
                                  alibi_slopes, lens.contiguous())
        return o
    o, _ = ref.attention_fwd(q, k, v, False, scale, alibi_slopes, lens)
    return o


def _qkv_views(qkv: torch.Tensor, num_heads: int):
    """The q, k, v [B,h,S,d] strided views of a packed [B,S,h*3*d] tensor
    (per-head [q|k|v] layout); no copies."""
    B, S, F = qkv.shape
    qkv5 = qkv.view(B, S, num_heads, 3, F // (3 * num_heads))
    return tuple(qkv5[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))


class _FlashAttentionQKV(torch.autograd.Function):
    """Packed-qkv attention: input [B, S, h*3d] (per-head [q|k|v] layout),
    output [B, S, h*d].  The strided gfx950 kernel reads/writes these
    layouts directly — zero permute/contiguous copies on the hot path."""

    @staticmethod
    def forward(ctx, qkv, num_heads, causal, scale):
        B, S, F = qkv.shape
        h = num_heads
        d = F // (3 * h)
        if scale is None:
            scale = 1.0 / math.sqrt(d)
        q, k, v = _qkv_views(qkv, h)
        if use_hip(qkv):
            o_buf = torch.empty(B, S, h * d, dtype=qkv.dtype,
                                device=qkv.device)
            o_view = o_buf.view(B, S, h, d).permute(0, 2, 1, 3)
            lse = torch.empty(B, h, S, dtype=torch.float32,
                              device=qkv.device)
            hip_ops().attn_fwd_out(q, k, v, o_view, lse, causal, scale)
        else:
            o4, lse = ref.attention_fwd(q.contiguous(), k.contiguous(),
                                        v.contiguous(), causal, scale)
            o_buf = o4.permute(0, 2, 1, 3).reshape(B, S, h * d)
        ctx.save_for_backward(qkv, o_buf, lse)
        ctx.meta = (num_heads, causal, scale)
        return o_buf

    @staticmethod
    def backward(ctx, do):
        qkv, o_buf, lse = ctx.saved_tensors
        h, causal, scale = ctx.meta
        B, S, F = qkv.shape
        d = F // (3 * h)
        q, k, v = _qkv_views(qkv, h)
        do4 = do.view(B, S, h, d).permute(0, 2, 1, 3)
        o4 = o_buf.view(B, S, h, d).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        dq_v, dk_v, dv_v = _qkv_views(dqkv, h)
        if use_hip(qkv):
            # fused MFMA bwd writes straight into the packed dqkv views
            hip_ops().attn_bwd_out(do4, q, k, v, o4, lse, dq_v, dk_v, dv_v,
                                   causal, scale)
        else:
            dq, dk, dv = ref.attention_bwd(
                do4.contiguous(), q.contiguous(), k.contiguous(),
                v.contiguous(), o4.contiguous(), lse, causal, scale)
            dq_v.copy_(dq)
            dk_v.copy_(dk)
            dv_v.copy_(dv)
        return dqkv, None, None, None


def flash_attention_qkv(qkv: torch.Tensor, num_heads: int,
                        causal: bool = True,
                        scale: Optional[float] = None) -> torch.Tensor:
    """Attention on the packed qkv projection output [B, S, heads*3*d]
    (per-head [q|k|v] blocks) -> [B, S, heads*d].  No layout copies."""
    return _FlashAttentionQKV.apply(qkv, num_heads, causal, scale)


class _SoftmaxCrossEntropy(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, targets):
        logits = logits.contiguous()
        if use_hip(logits):
            loss, lse = hip_ops().cross_entropy_fwd(logits, targets)
        else:
            loss, lse = ref.softmax_cross_entropy_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse = ctx.saved_tensors
        if use_hip(logits):
            dlogits = hip_ops().cross_entropy_bwd(dloss.contiguous(), logits,
                                                  targets, lse)
        else:
            dlogits = ref.softmax_cross_entropy_bwd(dloss, logits, targets, lse)
        return dlogits, None


def softmax_cross_entropy(logits: torch.Tensor,
                          targets: torch.Tensor) -> torch.Tensor:
    """Fused LM-head loss over the full vocab; logits [N, V], targets [N].

    Returns per-token loss [N] (caller reduces). Avoids materializing the
    softmax in fp32 [N, 51200].
    """
    return _SoftmaxCrossEntropy.apply(logits, targets)


# The loss over a vocab-sharded LM head, in three pieces that carry no
# autograd of their own: parallel.layers.fused_vocab_parallel_cross_entropy
# puts the one collective between the first two and is the autograd user.


def vocab_ce_fused_ok(logits: torch.Tensor) -> bool:
    """Envelope of the vocab-shard loss kernels (csrc/cross_entropy.hip; the
    bindings check the same): a contiguous 2-D bf16 shard on the GPU whose
    width is a multiple of 8 and whose data is 16-byte aligned, for the
    16-byte row loads."""
    if not (logits.is_cuda and logits.dtype == torch.bfloat16):
        return False
    if logits.dim() != 2 or not logits.is_contiguous():
        return False
    if logits.shape[-1] < 8 or logits.shape[-1] % 8 != 0 or \
            logits.data_ptr() % 16 != 0:
        return False
    return use_hip(logits)


@torch.no_grad()
def softmax_cross_entropy_partial(logits: torch.Tensor,
                                  targets: torch.Tensor,
                                  vocab_start: int) -> torch.Tensor:
    """Row statistics of one vocab shard, logits [N, Vs] = global columns
    [vocab_start, vocab_start + Vs), targets [N] global ids: stats [3, N]
    = (row max m, s = sum exp(x - m), t = target logit if the shard owns
    the target else 0).  A row of -inf only gives m = -inf, s = 0.  fp32 on
    the GPU: one read of the shard, bit-reproducible, no read-back, and a
    target outside the shard (negative or past the vocab too) is never
    used as an index."""
    if use_hip(logits):
        return hip_ops().cross_entropy_partial_fwd(
            logits.contiguous(), targets.contiguous(), int(vocab_start))
    return ref.softmax_cross_entropy_partial(logits, targets,
                                             int(vocab_start))


@torch.no_grad()
def softmax_cross_entropy_combine(stats: torch.Tensor):
    """stats [T, 3, N], the partial statistics of T shards in rank order ->
    (loss [N], lse [N]) over the whole vocab.  [N]-sized elementwise work
    in a fixed (rank) order on either device, so ranks holding the same
    gathered stats agree bit for bit.  A row that is -inf on every shard
    is undefined."""
    return ref.softmax_cross_entropy_combine(stats)


@torch.no_grad()
def softmax_cross_entropy_shard_bwd(dloss: torch.Tensor,
                                    logits: torch.Tensor,
                                    targets: torch.Tensor, lse: torch.Tensor,
                                    vocab_start: int) -> torch.Tensor:
    """dlogits [N, Vs] of one vocab shard from the whole-vocab lse [N]:
    (exp(x - lse) - onehot) * dloss, the one-hot only on the shard that
    owns the target.  A -inf logit gets exactly 0."""
    if use_hip(logits):
        return hip_ops().cross_entropy_shard_bwd(
            dloss.contiguous(), logits.contiguous(), targets.contiguous(),
            lse, int(vocab_start))
    return ref.softmax_cross_entropy_shard_bwd(dloss, logits, targets, lse,
                                               int(vocab_start))


# Columns per segment of the top-k kernels' partial pass: LS_BLOCK *
# LS_ROUNDS 16-byte groups in csrc/logits_sample.hip (the extension's
# logits_topk_segment reports them).  A function of the dtype alone.
LOGITS_TOPK_SEG = {torch.bfloat16: 8192, torch.float32: 4096}


def logits_topk_ok(logits: torch.Tensor, k: int) -> bool:
    """Envelope of the top-k log-prob and sampling kernels
    (csrc/logits_sample.hip; the bindings check the same): a 2-D bf16 or
    fp32 tensor on the GPU with 1..65535 rows, contiguous columns and every
    row 16-byte aligned (aligned base, row stride a multiple of 16 bytes: a
    column slice or a row-strided view is fine), and 1 <= k <= min(V, 128)."""
    if not (logits.is_cuda and logits.dim() == 2 and
            logits.dtype in LOGITS_TOPK_SEG):
        return False
    B, V = logits.shape
    if not (1 <= B <= 65535 and 1 <= k <= min(V, 128) and
            V <= 2 ** 31 - 8193 and logits.stride(1) == 1):
        return False
    per16 = 16 // logits.element_size()
    if logits.data_ptr() % 16 != 0 or (
            B > 1 and (logits.stride(0) < 0 or logits.stride(0) % per16)):
        return False
    return use_hip(logits)


def _row_param(value, B: int, dtype, device) -> torch.Tensor:
    """A per-row kernel parameter as a contiguous [B] device tensor."""
    if isinstance(value, torch.Tensor):
        return value.to(device=device, dtype=dtype).reshape(-1).expand(
            B).contiguous()
    return torch.full((B,), value, dtype=dtype, device=device)


@torch.no_grad()
def logits_topk(logits: torch.Tensor, k: int, inv_temperature=None,
                vocab_start: int = 0):
    """Top-k of a row of logits with its softmax statistics, in one read:
    logits [B, V], y = float(logits) * inv_temperature (a [B] tensor or a
    number, default 1; one fp32 multiply) -> (vals [B, k] fp32 = the k
    largest y, descending, equal y by lower column; idx [B, k] int64 =
    column + vocab_start; m [B] = max y; s [B] = sum exp(y - m)).  The
    log-probability of candidate j is vals[:, j] - m - log(s); over a vocab
    shard, (m, s) and the candidates combine across shards as the
    cross-entropy statistics do.  k is clamped to V.  A row of -inf only
    gives m = -inf, s = 0; a NaN makes m and s NaN and leaves idx in range.
    Inside logits_topk_ok this is the two gfx950 kernels (per-segment radix
    select, fixed-order merge): a row's output bits depend on that row
    alone, nothing is read back, so the call can be captured in a graph.
    On CPU or outside the envelope it is reference.logits_topk."""
    B, V = logits.shape
    k = min(int(k), V)
    if logits_topk_ok(logits, k):
        inv_t = _row_param(1.0 if inv_temperature is None else
                           inv_temperature, B, torch.float32, logits.device)
        return tuple(hip_ops().logits_topk(logits, k, inv_t,
                                           int(vocab_start)))
    inv_t = None if inv_temperature is None else _row_param(
        inv_temperature, B, torch.float32, logits.device)
    return ref.logits_topk(logits, k, inv_t, int(vocab_start))


@torch.no_grad()
def sample_logits(logits: torch.Tensor, u: torch.Tensor, inv_temperature,
                  top_k, top_p, k: int = 64) -> torch.Tensor:
    """One token [B] int64 per row of logits [B, V] by temperature / top-k /
    top-p sampling, every parameter per row ([B] tensors, or numbers shared
    by the rows): u uniform in [0, 1), inv_temperature > 0, top_k (0 or
    above k: all k candidates), top_p.  The candidates are logits_topk's k
    (clamped to V) with p_j = exp(y_j - y_0); the smallest prefix reaching
    top_p of their mass is kept (always candidate 0) and renormalised, and
    the token is the inverse CDF of the kept prefix at u.  top_k = 1 is the
    argmax with the lower column on a tie.  Inside logits_topk_ok the draw
    happens in the merge kernel's launch, with no read-back; on CPU or
    outside the envelope it is reference.sample_logits."""
    B, V = logits.shape
    k = min(int(k), V)
    dev = logits.device
    u = _row_param(u, B, torch.float32, dev)
    inv_t = _row_param(inv_temperature, B, torch.float32, dev)
    top_k = _row_param(top_k, B, torch.int32, dev)
    top_p = _row_param(top_p, B, torch.float32, dev)
    if logits_topk_ok(logits, k):
        return hip_ops().logits_topk(logits, k, inv_t, 0, u, top_k, top_p)[4]
    return ref.sample_logits(logits, u, inv_t, top_k, top_p, k)


_ADAM_CHUNK = 16384  # must match ADAM_CHUNK in csrc/adamw.hip
_ADAM_TILE = 64  # must match ADAM_TILE in csrc/adamw.hip
_ADAM_TABLE_CACHE: dict = {}


def _upload_tables(rows, dev):
    """rows: (p, g, m, v, numel, is_bf16, twin, rows | cols << 32) per
    tensor, pointers as ints; twin is 0 for a tensor without one.  Returns
    the device-side descriptor table and the chunk table that maps each
    workgroup to (tensor_idx, chunk_idx): one per started _ADAM_CHUNK
    elements, or one per _ADAM_TILE x _ADAM_TILE tile of a tensor with a
    twin (whose rows and cols are multiples of the tile)."""
    n = len(rows)
    descs = torch.tensor(rows, dtype=torch.int64).reshape(n, 8)
    counts = [r[4] // (_ADAM_TILE * _ADAM_TILE) if r[6] else
              (r[4] + _ADAM_CHUNK - 1) // _ADAM_CHUNK for r in rows]
    tensor_idx = torch.repeat_interleave(
        torch.arange(n, dtype=torch.int32),
        torch.tensor(counts, dtype=torch.int64))
    chunk_idx = torch.cat([torch.arange(c, dtype=torch.int32)
                           for c in counts])
    chunks = torch.stack([tensor_idx, chunk_idx], dim=1).contiguous()
    return descs.to(dev), chunks.to(dev)


def _adam_tables(params, grads, exp_avgs, exp_avg_sqs, twins=None):
    """Build (and cache) the device-side tensor-descriptor + chunk tables
    consumed by the multi-tensor AdamW kernel (one launch per step)."""
    if twins is None:
        twins = [None] * len(params)
    # the key covers every field a descriptor row holds: a second optimizer
    # over the same params brings new moment buffers, and the caching
    # allocator can hand the same base pointers to tensors of another
    # size or dtype
    key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                 p.numel(), p.dtype, 0 if t is None else t.data_ptr())
                for p, g, m, v, t in zip(params, grads, exp_avgs,
                                         exp_avg_sqs, twins))
    hit = _ADAM_TABLE_CACHE.get(key)
    if hit is not None:
        return hit
    rows = []
    for p, g, m, v, t in zip(params, grads, exp_avgs, exp_avg_sqs, twins):
        assert p.is_contiguous() and g.is_contiguous()
        assert m.dtype == torch.float32 and v.dtype == torch.float32
        assert p.dtype == g.dtype and p.dtype in (torch.bfloat16,
                                                  torch.float32)
        twin_ptr = shape = 0
        if t is not None:
            assert g.shape == p.shape
            if p.is_cuda:
                hip_ops().adamw_check_twin(p, m, v, t)
            twin_ptr = t.data_ptr()
            shape = p.shape[0] | (p.shape[1] << 32)
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                     p.numel(), 1 if p.dtype == torch.bfloat16 else 0,
                     twin_ptr, shape))
    tbl = _upload_tables(rows, params[0].device)
    _ADAM_TABLE_CACHE[key] = tbl
    return tbl


_SUMSQ_TABLE_CACHE: dict = {}


def _sumsq_tables(tensors):
    """Tables for the sum-of-squares kernels, in the AdamW layout with only
    the g, numel and is_bf16 fields filled, plus the per-chunk fp32
    workspace.  Built on the first call for a tensor list and cached, so
    later calls copy nothing to the device."""
    key = tuple((t.data_ptr(), t.numel(), t.dtype) for t in tensors)
    hit = _SUMSQ_TABLE_CACHE.get(key)
    if hit is not None:
        return hit
    rows = []
    for t in tensors:
        assert t.is_contiguous()
        assert t.dtype in (torch.bfloat16, torch.float32)
        rows.append((0, t.data_ptr(), 0, 0, t.numel(),
                     1 if t.dtype == torch.bfloat16 else 0, 0, 0))
    dev = tensors[0].device
    descs, chunks = _upload_tables(rows, dev)
    partials = torch.empty(chunks.shape[0], dtype=torch.float32, device=dev)
    tbl = (descs, chunks, partials)
    _SUMSQ_TABLE_CACHE[key] = tbl
    return tbl


@torch.no_grad()
def multi_tensor_sumsq(tensors: List[torch.Tensor]) -> torch.Tensor:
    """Sum of squares over every element of every tensor: fp32 [1] on the
    tensors' device.  The list may mix bf16 and fp32; each tensor is
    contiguous and may be a view at any element offset.

    On the GPU this is one reduce launch plus one finalize launch, with a
    fixed summation order (bit-reproducible) and no device read-back, so it
    can sit inside a captured graph after one eager call has built the
    cached tables.  The per-chunk workspace is shared by every call on the
    same tensor list, so such calls belong on one stream.  Its sqrt is the
    global norm that :func:`fused_adamw` clips by."""
    tensors = [t for t in tensors if t.numel() > 0]
    if not tensors:
        raise ValueError("multi_tensor_sumsq needs at least one element")
    if use_hip(tensors[0]):
        descs, chunks, partials = _sumsq_tables(tensors)
        out = torch.empty(1, dtype=torch.float32, device=tensors[0].device)
        hip_ops().multi_tensor_sumsq_raw(descs, chunks, partials, out)
        return out
    return ref.multi_tensor_sumsq(tensors)


@torch.no_grad()
def fused_adamw(params: List[torch.Tensor], grads: List[torch.Tensor],
                exp_avgs: List[torch.Tensor], exp_avg_sqs: List[torch.Tensor],
                step: int, lr: float, beta1: float = 0.9, beta2: float = 0.95,
                eps: float = 1e-8, weight_decay: float = 0.0,
                grad_scale: float = 1.0,
                grad_sumsq: Optional[torch.Tensor] = None,
                max_grad_norm: Optional[float] = None,
                twins: Optional[List[Optional[torch.Tensor]]] = None) -> None:
    """Multi-tensor AdamW update, in place — ONE kernel launch for all
    params.

    ``twins``, aligned with ``params``, gives for each parameter either
    None or a bf16 [cols, rows] tensor that receives the transpose of the
    updated [rows, cols] parameter in the same launch (see
    :func:`weight_twin_eligible` for which parameters can have one).  A
    step that changes nothing (non-finite norm, below) leaves it alone too.

    Params may be bf16 (fp32 master math happens inside the kernel against
    the fp32 exp_avg/exp_avg_sq state).  Analog of the fused Adam the
    reference gets inside its apply_grad HLO.

    Global-norm clipping (optax ``clip_by_global_norm``): give both
    ``grad_sumsq``, the fp32 [1] sum of squares of ALL gradients of the
    model (:func:`multi_tensor_sumsq`, summed over ranks where gradients
    are sharded), and ``max_grad_norm``.  The gradients are then scaled by
    ``grad_scale * max_grad_norm / max(norm, max_grad_norm)`` with
    ``norm = |grad_scale| * sqrt(grad_sumsq)``, inside the kernel: the
    coefficient never leaves the device.  If the norm is not finite the
    call changes nothing — params and moments keep their values — though
    the caller's step counter has moved on.  bf16 gradients above about
    1.8e19 overflow the fp32 square and count as non-finite.
    """
    if (grad_sumsq is None) != (max_grad_norm is None):
        raise ValueError(
            "grad_sumsq and max_grad_norm must be given together")
    if max_grad_norm is not None and not max_grad_norm > 0:
        raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
    if not params:
        return
    if twins is not None and len(twins) != len(params):
        raise ValueError("twins must be aligned with params")
    if use_hip(params[0]):
        descs, chunks = _adam_tables(params, grads, exp_avgs, exp_avg_sqs,
                                     twins)
        hip_ops().adamw_step_raw(descs, chunks, step, lr, beta1, beta2, eps,
                                 weight_decay, grad_scale, grad_sumsq,
                                 max_grad_norm or 0.0)
    else:
        ref.adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1,
                       beta2, eps, weight_decay, grad_scale, grad_sumsq,
                       max_grad_norm, twins)


# ------------------------------ weight twins ------------------------------
# A twin is a contiguous bf16 copy of W.t() for a linear weight W [out, in]:
# with it the dX GEMM dY @ W becomes dY @ twin.t(), the K-contiguous (TN)
# layout of the forward, which hipBLASLt runs 20-30 % faster than the NN
# layout (docs/BENCHMARK.md, "dX on weight twins").  It is derived state:
# it lives here, keyed weakly by the parameter, never in the module, and is
# kept current by the optimizer that registered it (fused_adamw writes it).

class _TwinEntry:
    """twin, and the state of the weight it was built from: its version
    counter and the address of its storage."""
    __slots__ = ("twin", "version", "ptr")

    def __init__(self, twin, w):
        self.twin = twin
        self.mark_current(w)

    def mark_current(self, w):
        self.version, self.ptr = w._version, w.data_ptr()

    def is_current(self, w):
        return self.version == w._version and self.ptr == w.data_ptr()


# id(parameter) -> entry, dropped when the parameter dies (a tensor cannot
# key a WeakKeyDictionary: its == is elementwise)
_WEIGHT_TWINS: dict = {}


def weight_twin_eligible(w: torch.Tensor) -> bool:
    """Can `w` have a twin: 2-D and contiguous, and on the GPU what the
    tiled path of the AdamW kernel asks for: bf16, 16-byte aligned, rows
    and cols multiples of its tile.  (The CPU reference takes any dtype and
    shape, so CPU runs go through the same plumbing.)"""
    if w.dim() != 2 or not w.is_contiguous() or not w.is_floating_point():
        return False
    if not w.is_cuda:
        return True
    return (w.dtype == torch.bfloat16 and w.data_ptr() % 16 == 0
            and w.shape[0] % _ADAM_TILE == 0 and w.shape[1] % _ADAM_TILE == 0)


@torch.no_grad()
def register_weight_twin(w: torch.Tensor) -> Optional[torch.Tensor]:
    """Allocate, fill and register the twin of `w`; None (and nothing
    allocated) if `w` is not eligible.  The caller takes on keeping it
    current: see :func:`weight_twin_written`."""
    if not weight_twin_eligible(w):
        return None
    entry = _WEIGHT_TWINS.get(id(w))
    if entry is None:
        entry = _TwinEntry(w.t().contiguous(), w)
        _WEIGHT_TWINS[id(w)] = entry
        weakref.finalize(w, _WEIGHT_TWINS.pop, id(w), None)
    return entry.twin


@torch.no_grad()
def weight_twin(w: torch.Tensor) -> Optional[torch.Tensor]:
    """The registered twin of `w`, current, or None if it has none.
    fused_adamw does not bump `w._version`; in-place writers that autograd
    sees (load_state_dict, a checkpoint restore, init, copy_) do, and a
    swap of the storage (`w.data = ...`, `model.to(...)`) moves
    `w.data_ptr()`; after either the twin is rebuilt here before it is
    handed out.  NOT caught: an in-place write through `w.data`
    (`w.data.copy_(...)`) and a second optimizer stepping `w` without
    twins; after those, call :func:`invalidate_weight_twin`.  During
    stream capture a rebuild would be baked into the graph and replayed
    every step, so a stale twin is an error there."""
    entry = _WEIGHT_TWINS.get(id(w))
    if entry is None:
        return None
    if not entry.is_current(w):
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "weight twin is stale during graph capture: the weight was "
                "written by something other than the optimizer step; call "
                "ops.weight_twin on it (or run one eager step) first")
        if entry.twin.device != w.device or entry.twin.dtype != w.dtype:
            entry.twin = w.t().contiguous()
        else:
            entry.twin.copy_(w.t())
        entry.mark_current(w)
    return entry.twin


def invalidate_weight_twin(w: torch.Tensor) -> None:
    """Mark the twin of `w` stale after a write that neither bumped
    `w._version` nor moved its storage."""
    entry = _WEIGHT_TWINS.get(id(w))
    if entry is not None:
        entry.version = -1


def weight_twin_written(w: torch.Tensor) -> None:
    """The twin of `w` was just written together with `w` by an op that
    does not bump `w._version` (fused_adamw): record that it is current."""
    entry = _WEIGHT_TWINS.get(id(w))
    if entry is not None:
        entry.mark_current(w)


def valid_weight_twin(w: torch.Tensor) -> Optional[torch.Tensor]:
    """The twin a dX GEMM should read in place of `w`: :func:`weight_twin`,
    or None when global_config.weight_twin is off.  The optimizer keeps the
    twin up whatever the switch says, so it can be flipped at any time."""
    from ..global_env import global_config
    return weight_twin(w) if global_config.weight_twin else None


# ------------------------------- MoE routing -------------------------------


class MoERouting(NamedTuple):
    """Result of :func:`moe_top2_route` for N tokens, E experts, capacity C.

    w1, w2 [N] gate weights (normalised before capacity drops); idx1, idx2
    [N] chosen experts; slot1, slot2 [N] slot in the [E*C] dispatch buffer
    or -1 when dropped; src [E*C] token in each slot or -1; aux_loss the
    GShard load-balance loss.  Integer fields are int32 and carry no
    gradient."""
    w1: torch.Tensor
    w2: torch.Tensor
    idx1: torch.Tensor
    idx2: torch.Tensor
    slot1: torch.Tensor
    slot2: torch.Tensor
    src: torch.Tensor
    aux_loss: torch.Tensor


class _MoeTop2Route(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, capacity):
        logits = logits.contiguous()
        if use_hip(logits):
            outs = hip_ops().moe_route_fwd(logits, capacity)
        else:
            outs = ref.moe_top2_route(logits, capacity)
        w1, w2, idx1, idx2, slot1, slot2, src, aux, count1 = outs
        ctx.save_for_backward(logits, idx1, idx2, w1, w2, count1)
        ctx.mark_non_differentiable(idx1, idx2, slot1, slot2, src)
        return w1, w2, idx1, idx2, slot1, slot2, src, aux

    @staticmethod
    def backward(ctx, dw1, dw2, _i1, _i2, _s1, _s2, _src, daux):
        logits, idx1, idx2, w1, w2, count1 = ctx.saved_tensors
        if use_hip(logits):
            return hip_ops().moe_route_bwd(
                logits, idx1, idx2, w1, w2, count1, dw1.float().contiguous(),
                dw2.float().contiguous(), daux.float().contiguous()), None
        return ref.moe_top2_route_bwd(logits, idx1, idx2, w1, w2, count1,
                                      dw1, dw2, daux), None


def moe_top2_route(logits: torch.Tensor, capacity: int) -> MoERouting:
    """Top-2 gate + capacity slot assignment over logits [N, E].

    Token order decides who keeps a slot, the lowest expert index wins a
    tie, and every output shape depends on (N, E, capacity) only — the op
    never reads the device back, so it can sit inside a captured graph.
    Gradients flow to logits through w1, w2 and aux_loss."""
    return MoERouting(*_MoeTop2Route.apply(logits, int(capacity)))


class _MoeDispatch(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, src, slot1, slot2):
        x = x.contiguous()
        ctx.save_for_backward(slot1, slot2)
        if use_hip(x):
            return hip_ops().moe_dispatch(x, src)
        return ref.moe_dispatch(x, src)

    @staticmethod
    def backward(ctx, g):
        slot1, slot2 = ctx.saved_tensors
        if use_hip(g):
            dx = hip_ops().moe_combine(g.contiguous(), None, None, slot1,
                                       slot2)
        else:
            dx = ref.moe_dispatch_bwd(g, slot1, slot2)
        return dx, None, None, None


def moe_dispatch(x: torch.Tensor, routing: MoERouting) -> torch.Tensor:
    """x [N, H] -> [E*C, H]: slot s holds x[routing.src[s]], empty slots
    are zero.  One gather pass; backward is a gather too."""
    return _MoeDispatch.apply(x, routing.src, routing.slot1, routing.slot2)


class _MoeCombine(torch.autograd.Function):

    @staticmethod
    def forward(ctx, y, w1, w2, slot1, slot2, src):
        y = y.contiguous()
        ctx.save_for_backward(y, w1, w2, slot1, slot2, src)
        if use_hip(y):
            return hip_ops().moe_combine(y, w1.float().contiguous(),
                                         w2.float().contiguous(), slot1,
                                         slot2)
        return ref.moe_combine(y, w1, w2, slot1, slot2)

    @staticmethod
    def backward(ctx, dout):
        y, w1, w2, slot1, slot2, src = ctx.saved_tensors
        if use_hip(y):
            dout = dout.contiguous()
            dy = hip_ops().moe_dispatch(dout, src, slot1,
                                        w1.float().contiguous(),
                                        w2.float().contiguous())
            dw1, dw2 = hip_ops().moe_combine_dw(dout, y, slot1, slot2)
            dw1, dw2 = dw1.to(w1.dtype), dw2.to(w2.dtype)
        else:
            dy, dw1, dw2 = ref.moe_combine_bwd(dout, y, w1, w2, slot1,
                                               slot2, src)
        return dy, dw1, dw2, None, None, None


def moe_combine(y: torch.Tensor, routing: MoERouting) -> torch.Tensor:
    """y [E*C, H] -> [N, H]: out[t] = w1*y[slot1[t]] + w2*y[slot2[t]] with
    dropped choices skipped; fp32 sum, rounded once.  Gradients flow to y
    and to the gate weights."""
    return _MoeCombine.apply(y, routing.w1, routing.w2, routing.slot1,
                             routing.slot2, routing.src)


def moe_fused_ok(x: torch.Tensor, num_experts: int,
                 capacity: Optional[int] = None) -> bool:
    """Envelope of the HIP routing kernels (csrc/moe_route.hip; the
    bindings check the same): bf16 on the GPU, H % 8 == 0 for the 16-byte
    row accesses, 2 <= E <= 128, E * capacity < 2^31."""
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if x.shape[-1] < 8 or x.shape[-1] % 8 != 0 or \
            not 2 <= num_experts <= 128:
        return False
    if capacity is not None and num_experts * capacity >= 2 ** 31:
        return False
    return use_hip(x)


# ----------------------------- skinny decode GEMM --------------------------

def _skinny_mt(M: int) -> int:
    """The kernel's padded-M tier: the power of two >= max(M, 4)."""
    MT = 4
    while MT < M:
        MT *= 2
    return MT


def _skinny_legal_splits(K: int, MT: int, fp4: bool = False) -> List[int]:
    """Ascending split-K factors the kernel takes: s divides K/64 (keeps
    rounds = K/8/s a multiple of the 8-deep pipeline) and the LDS x-slice
    (rounds * 16 * MT bytes) fits 64 KB.  The MXFP4 kernel
    (csrc/skinny_fp4.hip) walks 32-k scale blocks in rounds of 8: K % 256 == 0,
    s divides K/256, up to 8 tokens, the same LDS rule."""
    if fp4 and (K <= 0 or K % 256 or MT > 8):
        return []
    q = K // (256 if fp4 else 64)
    return [s for s in range(1, q + 1)
            if q % s == 0 and (K // 8 // s) * 16 * MT <= 65536]


@functools.lru_cache(maxsize=None)
def _skinny_splits(N: int, K: int, M: int, fp4: bool = False) -> Optional[int]:
    """Split-K factor for the decode GEMV: a legal split
    (_skinny_legal_splits) whose grid (N/64 x s) should fill the 256 CUs.
    None = shapes unsupported."""
    lds_ok = _skinny_legal_splits(K, _skinny_mt(M), fp4)
    if not lds_ok:
        return None
    # sweep-tuned (tools/skinny_bench.py): ~16 k-rounds per workgroup is
    # the sweet spot — take the LARGEST split with rounds >= 16 that
    # still fills the chip, else the most-parallel legal config
    for s in sorted(lds_ok, reverse=True):
        if K // 8 // s >= 16 and (N // 64) * s >= 1024:
            return s
    for s in lds_ok:
        if (N // 64) * s >= 2560:
            return s
    return lds_ok[-1]


#: LDS bytes the MFMA kernel's staged x slice may take (SKINNY_MFMA_LDS_MAX
#: in csrc/launchers.h: the CU's 160 KB)
_SKINNY_MFMA_LDS = 160 * 1024


def _skinny_mfma_mt(M: int) -> int:
    """The MFMA kernel's token tier: 16, 32 or 64."""
    return 16 if M <= 16 else 32 if M <= 32 else 64


def _skinny_mfma_legal_splits(K: int, MT: int) -> List[int]:
    """Ascending split-K factors the MFMA kernel takes: K % 256 == 0, s
    divides K/256 (a k-slice is whole 8-k-step pipeline rounds) and the
    LDS x slice MT * (K/s + 16) * 2 bytes fits _SKINNY_MFMA_LDS."""
    if K <= 0 or K % 256:
        return []
    q = K // 256
    return [s for s in range(1, q + 1)
            if q % s == 0 and MT * (K // s + 16) * 2 <= _SKINNY_MFMA_LDS]


@functools.lru_cache(maxsize=None)
def _skinny_mfma_splits(N: int, K: int, M: int) -> Optional[int]:
    """Split-K factor for the MFMA skinny GEMM (grid ceil(N/256) x s
    workgroups of 4 waves): a legal split (_skinny_mfma_legal_splits).
    None = outside the kernel's envelope."""
    if not 9 <= M <= 64 or N <= 0 or N % 64:
        return None
    legal = _skinny_mfma_legal_splits(K, _skinny_mfma_mt(M))
    if not legal:
        return None
    wgs = -(-N // 256)
    # same two-rule shape as _skinny_splits, thresholds from the
    # tools/skinny_bench.py sweep (docs/BENCHMARK.md): the best split of
    # every swept shape has 100-400 workgroups and k-slices of 512-2048 --
    # every further split adds M*N*4 bytes of partials to write and read
    # back.  So: the SMALLEST split with >= 192 workgroups (3/4 of the 256
    # CUs) and k-slices <= 2048, else the smallest that fills alone
    for s in legal:
        if wgs * s >= 192 and K // s <= 2048:
            return s
    for s in legal:
        if wgs * s >= 192:
            return s
    return legal[-1]


#: the weight format of the packed decode kernels as the pack and tuning keys
#: carry it: False = bf16, True = e4m3 with one scale, "mxfp4"
_MXFP4 = "mxfp4"


def _skinny_fmt(module):
    """The format skinny_linear packs this module's weight in (see _MXFP4):
    weight_fp4 before fp8_gemm, and neither for an _fp8_exclude module."""
    from ..global_env import global_config
    if getattr(module, "_fp8_exclude", False):
        return False
    if global_config.weight_fp4:
        return _MXFP4
    return bool(global_config.fp8_gemm)


def mxfp4_quantize(w: torch.Tensor):
    """w [N, K], K % 32 == 0 -> (codes uint8 [N, K/2], scales uint8
    [N, K/32]) by the OCP MX rule: per block of 32 along K the e8m0 byte
    E = clamp(floor(log2(amax)) - 2 + 127, 2, 252) (127 for a block of
    zeros), every element x / 2^(E-127) rounded to the nearest e2m1 value,
    ties to even, saturating at +-6, as sign<<3 | exp<<1 | mant with the even
    k in the low nibble.  ValueError on a non-finite weight.  Plain torch on
    the weight's device (reference.mxfp4_quantize): it runs once per weight."""
    return ref.mxfp4_quantize(w)


def mxfp4_dequantize(codes: torch.Tensor, scales: torch.Tensor,
                     dtype=torch.bfloat16) -> torch.Tensor:
    """The exact [N, K] weights that (codes, scales) of mxfp4_quantize stand
    for; every value is a normal bf16.  Either device."""
    return ref.mxfp4_dequantize(codes, scales, dtype)


def mxfp4_pack(codes: torch.Tensor, scales: torch.Tensor):
    """(codes [N, K/2], scales [N, K/32]), K % 256 == 0, in the one layout
    both MXFP4 kernels read (csrc/skinny_fp4.h): wq [K/32, N, 16], a 16-byte
    unit per row and scale block, and sq [K/256, N, 8], the 8 scale bytes of a
    row's 256 k."""
    N, K = codes.shape[0], codes.shape[1] * 2
    assert K % 256 == 0 and scales.shape == (N, K // 32)
    wq = codes.view(N, K // 32, 16).permute(1, 0, 2).contiguous()
    sq = scales.view(N, K // 256, 8).permute(1, 0, 2).contiguous()
    return wq, sq


def _skinny_cache(module, weight: torch.Tensor, fmt):
    """Packed weight and its scales, cached on the module and keyed on the
    parameter version (in-place optimizer updates bump it) and the format
    fmt (see _MXFP4): [K/8, N, 8] bf16 and None, e4m3 bytes and the fp32
    scale, or mxfp4_pack's (wq, sq)."""
    key = (weight._version, fmt)
    cached = getattr(module, "_skinny_pack", None)
    if cached is not None and cached[0] == key:
        return cached[1], cached[2]
    N, K = weight.shape
    with torch.no_grad():
        w = weight.contiguous()
        if fmt == _MXFP4:
            wp, scale = mxfp4_pack(*mxfp4_quantize(w))
        elif fmt:
            amax = w.abs().amax().float().clamp_min(1e-12)
            scale = (amax / 448.0).reshape(1)
            q = (w.float() / scale).clamp(-448.0, 448.0).to(
                torch.float8_e4m3fn)
            wp = q.view(torch.uint8).view(N, K // 8, 8) \
                .permute(1, 0, 2).contiguous()
        else:
            scale = None
            wp = w.view(N, K // 8, 8).permute(1, 0, 2).contiguous()
    module._skinny_pack = (key, wp, scale)
    return wp, scale


def _skinny_mfma_auto(N: int, K: int, M: int, fp8: bool) -> bool:
    """Where "auto" routes 9..64 tokens to the MFMA kernel: the shape
    classes and token tiers in which tools/skinny_bench.py measured it
    faster than the library's bf16 GEMM by more than the 6 % run-to-run
    spread (table in docs/BENCHMARK.md, rule on global_config.skinny_gemm).
      - K >= 2N (ffn down-projections, 5120 x 20480): every tier, bf16
        1.66-1.90x, e4m3 2.12-2.95x.
      - e4m3 weights otherwise: tiers 16 and 32 (1.15-2.69x on all five
        other shapes); tier 64 stays on the library (0.81-1.09x).
      - bf16 otherwise: tiers 16 and 32 at N <= K (5120 x 5120: 1.16-
        1.34x).  N > K (qkv, fc1) stays on the library: 0.81-0.98x, but
        for 20480 x 5120 at M = 16 (1.78x against a library outlier that
        M < 16 was not measured for).  Tier 64 stays too (0.66-0.98x)."""
    if K >= 2 * N:
        return True
    if M > 32:
        return False
    return fp8 or N <= K


def skinny_ok(x: torch.Tensor, weight: torch.Tensor, module=None) -> bool:
    """Gate for the packed decode kernels, inference only.  Up to 8 tokens:
    the dot2 GEMV (csrc/skinny_gemm.hip), 64-aligned dims.  Measured
    (tools/skinny_bench.py sweep): it wins 1.5-3.1x at M<=4-8 (up to
    6.2 TB/s bf16 / 4.6 TB/s-of-fp8-bytes) but the per-m VALU work makes
    M >= 16 issue-bound (SIMD-32 units: 2 cyc/VALU instr for wave64).
    9..64 tokens: the MFMA 16x16x32 kernel (csrc/skinny_mfma.hip) inside
    its envelope (N % 64 == 0, K % 256 == 0, a legal split); in "auto"
    only where _skinny_mfma_auto says it was measured to win.  Under
    global_config.weight_fp4 the module's format is MXFP4 (_skinny_fmt) and
    the gate is that of its two kernels (csrc/skinny_fp4.hip,
    csrc/skinny_mfma_fp4.hip: K % 256 == 0 at every token count); "auto"
    treats it as e4m3 (measured at hidden 5120, by analogy at hidden >= 7168:
    global_config.weight_fp4)."""
    from ..global_env import global_config
    mode = global_config.skinny_gemm
    if mode in ("0", False) or torch.is_grad_enabled():
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if torch.cuda.is_current_stream_capturing() and \
            getattr(module, "_skinny_pack", None) is None:
        # packing mustn't be captured into the graph; the warmup pass
        # before capture builds the cache, after which replay just
        # re-reads the packed weights in place
        return False
    N, K = weight.shape
    if mode == "auto" and (K > 6144 and N > 6144):
        # bf16 is outside the measured win envelope at hidden >= 7168
        # (hipBLASLt already streams >= 5 TB/s there), but the
        # fp8-PACKED variant reads half the bytes and wins end-to-end
        # (OPT-66B fp8 decode 25.4 vs 28.99 ms/token measured)
        if not _skinny_fmt(module):
            return False
    m = x.numel() // x.shape[-1]
    if m <= 8:
        return (N % 64 == 0 and K % 64 == 0
                and _skinny_splits(N, K, m, _skinny_fmt(module) == _MXFP4)
                is not None)
    # 9..64 tokens: the MFMA kernel, inside its envelope (and, in auto,
    # inside the measured win envelope: see global_config.skinny_gemm)
    if _skinny_mfma_splits(N, K, m) is None or x.data_ptr() % 16:
        return False
    if mode != "auto":
        return True
    return _skinny_mfma_auto(N, K, m, bool(_skinny_fmt(module)))


_SKINNY_TUNED = {}


def _skinny_gemm(kernel: str, fp4: bool):
    """The binding of one kernel ("dot2" or "mfma") and weight format as
    f(wp, x, scale, bias, N, K, splits); for MXFP4, wp and scale are
    mxfp4_pack's wq and sq."""
    ops = hip_ops()
    if not fp4:
        return ops.skinny_gemm_mfma if kernel == "mfma" else ops.skinny_gemm
    gemm = ops.skinny_gemm_mfma_fp4 if kernel == "mfma" else ops.skinny_gemm_fp4
    return lambda wq, x, sq, b, N, K, s: gemm(wq, sq, x, b, N, K, s)


def _skinny_tune(wp, x2, scale, N, K, MT, kernel="dot2", fp4=False):
    """One-time per-(shape, MT, dtype, kernel) split autotune: the best
    split factor is shape- AND M-dependent (measured: rounds=16 wins 66B
    fp8 decode, the fill-first choice wins 13B batch-1), so time the legal
    candidates once and cache — the ~2 ms cost amortizes over the
    decode loop, like a library heuristic cache.  `kernel` is "dot2"
    (skinny_gemm, MT its padded tier) or "mfma" (skinny_gemm_mfma, MT its
    token tier); the tag keeps their equal tiers apart in the cache.  The
    key's format entry is False (bf16), True (e4m3) or "mxfp4" (fp4=True,
    wp and scale being mxfp4_pack's wq and sq)."""
    key = (N, K, MT, _MXFP4 if fp4 else scale is not None, kernel)
    got = _SKINNY_TUNED.get(key)
    if got is not None:
        return got
    gemm = _skinny_gemm(kernel, fp4)
    if kernel == "mfma":
        legal = _skinny_mfma_legal_splits(K, MT)
        wgs = -(-N // 256)
        picks = (
            next((c for c in legal
                  if wgs * c >= 192 and K // c <= 2048), None),
            next((c for c in legal if wgs * c >= 96), None),
            next((c for c in legal if wgs * c >= 384), None),
            legal[-1])
    else:
        legal = _skinny_legal_splits(K, MT, fp4)
        picks = (
            next((c for c in reversed(legal)
                  if K // 8 // c >= 16 and (N // 64) * c >= 1024), None),
            next((c for c in legal if (N // 64) * c >= 2560), None),
            next((c for c in legal if K // 8 // c <= 32), None),
            legal[-1])
    cands = sorted({s for s in picks if s is not None})
    if len(cands) == 1:
        _SKINNY_TUNED[key] = cands[0]
        return cands[0]
    best, best_t = cands[0], float("inf")
    for c in cands:
        gemm(wp, x2, scale, None, N, K, c)  # warm
        t0 = torch.cuda.Event(True)
        t1 = torch.cuda.Event(True)
        t0.record()
        for _ in range(10):
            gemm(wp, x2, scale, None, N, K, c)
        t1.record()
        t1.synchronize()
        dt = t0.elapsed_time(t1)
        if dt < best_t:
            best, best_t = c, dt
    _SKINNY_TUNED[key] = best
    return best


def skinny_linear(x: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor], module) -> torch.Tensor:
    """y = x @ W^T (+bias) through the packed decode kernels: the dot2
    GEMV up to 8 tokens, the MFMA skinny GEMM for 9..64.  The weights are
    packed once per module (_skinny_cache) as bf16, as e4m3 with one scale
    (half the bytes/token) under global_config.fp8_gemm, or as MXFP4 (e2m1
    nibbles and e8m0 block scales, 4.25 bits a weight, dequantized exactly
    in registers) under global_config.weight_fp4, which goes first; a module
    marked _fp8_exclude stays bf16.  Split-K fp32 partials are stored and
    reduced in a fixed order by a finalize launch (deterministic, no
    atomics).  Inference only; on the CPU see reference.skinny_linear_fp4."""
    fmt = _skinny_fmt(module)
    fp4 = fmt == _MXFP4
    wp, scale = _skinny_cache(module, weight, fmt)
    N, K = weight.shape
    shape = x.shape
    x2 = x.reshape(-1, K).contiguous()
    b = bias.contiguous() if bias is not None else None
    M = x2.shape[0]
    # up to 8 tokens: the dot2 kernel; 9..64 (skinny_ok has checked the
    # envelope): the MFMA kernel, over the same packed weights
    if M <= 8:
        kernel, MT = "dot2", _skinny_mt(M)
        rule = functools.partial(_skinny_splits, fp4=fp4)
    else:
        kernel, MT, rule = "mfma", _skinny_mfma_mt(M), _skinny_mfma_splits
    if torch.cuda.is_current_stream_capturing():
        splits = _SKINNY_TUNED.get(
            (N, K, MT, _MXFP4 if fp4 else scale is not None, kernel)) \
            or rule(N, K, M)
    else:
        splits = _skinny_tune(wp, x2, scale, N, K, MT, kernel, fp4)
    y = _skinny_gemm(kernel, fp4)(wp, x2, scale, b, N, K, splits)
    return y.reshape(*shape[:-1], N)
