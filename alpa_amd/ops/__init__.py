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
for every decode step.

Kernel-level contract mirrors the reference's compiled-HLO op inventory
(GEMM+epilogue, attention, LayerNorm, fused Adam,
grad accumulation, collectives).
"""
from __future__ import annotations

import functools
import math
from typing import List, NamedTuple, Optional

import torch

from . import reference as ref
from ._backend import hip_ops, hip_ops_available, use_hip

__all__ = [
    "layer_norm", "add_layer_norm", "bias_gelu", "add_layer_norm_fp8",
    "bias_gelu_fp8", "flash_attention",
    "flash_attention_qkv", "flash_attention_decode", "decode_attn_ok",
    "DECODE_ATTN_CHUNK", "softmax_cross_entropy",
    "softmax_cross_entropy_partial", "softmax_cross_entropy_combine",
    "softmax_cross_entropy_shard_bwd", "vocab_ce_fused_ok", "fused_adamw",
    "multi_tensor_sumsq",
    "hip_ops_available", "MoERouting", "moe_top2_route", "moe_dispatch",
    "moe_combine", "moe_fused_ok",
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
    """y = x @ w.T + bias via torch.addmm: hipBLASLt fuses the bias
    epilogue into the GEMM (measured free — matmul+separate add cost
    ~16 ms per GPT-2.6B step, tools/addmm_probe.py).  Backward runs the
    standard dX/dW GEMMs and the HIP column-sum for db."""

    @staticmethod
    def forward(ctx, x, w, bias):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        y = torch.addmm(bias, x2, w.t())
        ctx.save_for_backward(x2, w)
        ctx.bias_dtype = bias.dtype
        return y.reshape(*shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x2, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        dx = (g2 @ w).reshape(*g.shape[:-1], w.shape[1])
        dw = g2.t() @ x2
        if use_hip(g2) and g2.dtype == torch.bfloat16:
            db = _colsum(g2, ctx.bias_dtype)
        else:
            db = g2.sum(0).to(ctx.bias_dtype)
        return dx, dw, db


def linear_bias(x: torch.Tensor, w: torch.Tensor,
                bias: torch.Tensor) -> torch.Tensor:
    """F.linear with the bias fused into the hipBLASLt epilogue and the
    bias grad on the HIP column-sum."""
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


def decode_attn_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Envelope of the split-KV decode attention kernel
    (csrc/attention_decode.hip; the binding checks the same): bf16 on the
    GPU, q [B, h, 1, d] and k, v [B, h, Skv, d] views with a contiguous
    head dim, d a multiple of 16 up to 256, and every row 16-byte aligned
    (aligned base, batch/head/seq strides multiples of 8 elements) for the
    16-byte loads."""
    for t in (q, k, v):
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
                and t.stride(3) == 1):
            return False
    D = q.shape[3]
    if q.shape[2] != 1 or D % 16 != 0 or not 16 <= D <= 256:
        return False
    if k.shape != v.shape or k.shape[:2] != q.shape[:2] or k.shape[3] != D \
            or q.shape[0] * q.shape[1] > 65535:
        return False
    if not all(_rows_aligned16(t) for t in (q, k, v)):
        return False
    return use_hip(q)


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


_ADAM_CHUNK = 16384  # must match ADAM_CHUNK in csrc/adamw.hip
_ADAM_TABLE_CACHE: dict = {}


def _upload_tables(rows, dev):
    """rows: (p, g, m, v, numel, is_bf16) per tensor, pointers as ints.
    Returns the device-side descriptor table and the chunk table that maps
    each workgroup to (tensor_idx, chunk_idx)."""
    n = len(rows)
    descs = torch.tensor(rows, dtype=torch.int64).reshape(n, 6)
    counts = [(r[4] + _ADAM_CHUNK - 1) // _ADAM_CHUNK for r in rows]
    tensor_idx = torch.repeat_interleave(
        torch.arange(n, dtype=torch.int32),
        torch.tensor(counts, dtype=torch.int64))
    chunk_idx = torch.cat([torch.arange(c, dtype=torch.int32)
                           for c in counts])
    chunks = torch.stack([tensor_idx, chunk_idx], dim=1).contiguous()
    return descs.to(dev), chunks.to(dev)


def _adam_tables(params, grads, exp_avgs, exp_avg_sqs):
    """Build (and cache) the device-side tensor-descriptor + chunk tables
    consumed by the multi-tensor AdamW kernel (one launch per step)."""
    # the key covers every field a descriptor row holds: a second optimizer
    # over the same params brings new moment buffers, and the caching
    # allocator can hand the same base pointers to tensors of another
    # size or dtype
    key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                 p.numel(), p.dtype)
                for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs))
    hit = _ADAM_TABLE_CACHE.get(key)
    if hit is not None:
        return hit
    rows = []
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        assert p.is_contiguous() and g.is_contiguous()
        assert m.dtype == torch.float32 and v.dtype == torch.float32
        assert p.dtype == g.dtype and p.dtype in (torch.bfloat16,
                                                  torch.float32)
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                     p.numel(), 1 if p.dtype == torch.bfloat16 else 0))
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
                     1 if t.dtype == torch.bfloat16 else 0))
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
                max_grad_norm: Optional[float] = None) -> None:
    """Multi-tensor AdamW update, in place — ONE kernel launch for all
    params.

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
    if use_hip(params[0]):
        descs, chunks = _adam_tables(params, grads, exp_avgs, exp_avg_sqs)
        hip_ops().adamw_step_raw(descs, chunks, step, lr, beta1, beta2, eps,
                                 weight_decay, grad_scale, grad_sumsq,
                                 max_grad_norm or 0.0)
    else:
        ref.adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1,
                       beta2, eps, weight_decay, grad_scale, grad_sumsq,
                       max_grad_norm)


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


def _skinny_legal_splits(K: int, MT: int) -> List[int]:
    """Ascending split-K factors the kernel takes: s divides K/64 (keeps
    rounds = K/8/s a multiple of the 8-deep pipeline) and the LDS x-slice
    (rounds * 16 * MT bytes) fits 64 KB."""
    q = K // 64
    return [s for s in range(1, q + 1)
            if q % s == 0 and (K // 8 // s) * 16 * MT <= 65536]


@functools.lru_cache(maxsize=None)
def _skinny_splits(N: int, K: int, M: int) -> Optional[int]:
    """Split-K factor for the decode GEMV: a legal split
    (_skinny_legal_splits) whose grid (N/64 x s) should fill the 256 CUs.
    None = shapes unsupported."""
    lds_ok = _skinny_legal_splits(K, _skinny_mt(M))
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


def _skinny_cache(module, weight: torch.Tensor, fp8: bool):
    """Packed [K/8, N, 8] weight (+ e4m3 scale), cached on the module and
    keyed on the parameter version (in-place optimizer updates bump it)."""
    key = (weight._version, fp8)
    cached = getattr(module, "_skinny_pack", None)
    if cached is not None and cached[0] == key:
        return cached[1], cached[2]
    N, K = weight.shape
    with torch.no_grad():
        w = weight.contiguous()
        if fp8:
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


def skinny_ok(x: torch.Tensor, weight: torch.Tensor, module=None) -> bool:
    """Gate for the decode GEMV kernel (csrc/skinny_gemm.hip): inference
    only, M <= 8 tokens, 64-aligned dims.  Measured (tools/
    skinny_bench.py sweep): the kernel wins 1.5-3.1x at M<=4-8 (up to
    6.2 TB/s bf16 / 4.6 TB/s-of-fp8-bytes) but the per-m VALU work makes
    M >= 16 issue-bound (SIMD-32 units: 2 cyc/VALU instr for wave64) —
    hipBLASLt keeps those; an MFMA 16x16x32 variant is the next step."""
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
        fp8 = (global_config.fp8_gemm and
               not getattr(module, "_fp8_exclude", False))
        if not fp8:
            return False
    m = x.numel() // x.shape[-1]
    return (m <= 8 and N % 64 == 0 and K % 64 == 0
            and _skinny_splits(N, K, m) is not None)


_SKINNY_TUNED = {}


def _skinny_tune(wp, x2, scale, N, K, MT):
    """One-time per-(shape, MT, dtype) split autotune: the best split
    factor is shape- AND M-dependent (measured: rounds=16 wins 66B fp8
    decode, the fill-first choice wins 13B batch-1), so time the legal
    candidates once and cache — the ~2 ms cost amortizes over the
    decode loop, like a library heuristic cache."""
    key = (N, K, MT, scale is not None)
    got = _SKINNY_TUNED.get(key)
    if got is not None:
        return got
    legal = _skinny_legal_splits(K, MT)
    cands = sorted({
        s for s in (
            next((c for c in reversed(legal)
                  if K // 8 // c >= 16 and (N // 64) * c >= 1024), None),
            next((c for c in legal if (N // 64) * c >= 2560), None),
            next((c for c in legal if K // 8 // c <= 32), None),
            legal[-1]) if s is not None})
    if len(cands) == 1:
        _SKINNY_TUNED[key] = cands[0]
        return cands[0]
    best, best_t = cands[0], float("inf")
    for c in cands:
        hip_ops().skinny_gemm(wp, x2, scale, None, N, K, c)  # warm
        t0 = torch.cuda.Event(True)
        t1 = torch.cuda.Event(True)
        t0.record()
        for _ in range(10):
            hip_ops().skinny_gemm(wp, x2, scale, None, N, K, c)
        t1.record()
        t1.synchronize()
        dt = t0.elapsed_time(t1)
        if dt < best_t:
            best, best_t = c, dt
    _SKINNY_TUNED[key] = best
    return best


def skinny_linear(x: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor], module) -> torch.Tensor:
    """y = x @ W^T (+bias) through the packed decode GEMV.  fp8 weights
    (half the bytes/token) when global_config.fp8_gemm is on and the
    module isn't _fp8_exclude; split-K fp32 partials are stored and
    reduced in a fixed order by a finalize launch (deterministic, no
    atomics).  Inference only."""
    from ..global_env import global_config
    fp8 = (global_config.fp8_gemm and
           not getattr(module, "_fp8_exclude", False))
    wp, scale = _skinny_cache(module, weight, fp8)
    N, K = weight.shape
    shape = x.shape
    x2 = x.reshape(-1, K).contiguous()
    b = bias.contiguous() if bias is not None else None
    MT = _skinny_mt(x2.shape[0])
    if torch.cuda.is_current_stream_capturing():
        splits = _SKINNY_TUNED.get((N, K, MT, scale is not None)) \
            or _skinny_splits(N, K, x2.shape[0])
    else:
        splits = _skinny_tune(wp, x2, scale, N, K, MT)
    y = hip_ops().skinny_gemm(wp, x2, scale, b, N, K, splits)
    return y.reshape(*shape[:-1], N)
