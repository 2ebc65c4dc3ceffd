"""Pure-PyTorch reference implementations of every hot op.

These serve two purposes:
1. CPU execution path (GPU-free unit tests, gloo multi-process tests).
2. Numerics oracle for the HIP kernels (tests compare the gfx950 kernel
   against these in fp32; see tests/test_kernels_gpu.py).

They are *not* used on a GPU box — `alpa_amd.ops` raises if the HIP extension
is missing there (anti-silent-fallback), unless explicitly overridden.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
import torch.nn.functional as F



def _up(t: torch.Tensor) -> torch.Tensor:
    """Upcast half-precision to fp32 for math; leave fp32/fp64 alone."""
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.float()
    return t

def layer_norm_fwd(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                   eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (y, mean, rstd). mean/rstd are fp32 per-row stats."""
    xf = _up(x)
    mean = xf.mean(dim=-1)
    var = xf.var(dim=-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    y = y * _up(weight) + _up(bias)
    return y.to(x.dtype), mean, rstd


def layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
                   mean: torch.Tensor, rstd: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (dx, dweight, dbias)."""
    xf = _up(x)
    dyf = _up(dy)
    xhat = (xf - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    wdy = dyf * _up(weight)
    H = x.shape[-1]
    c1 = wdy.mean(dim=-1, keepdim=True)
    c2 = (wdy * xhat).mean(dim=-1, keepdim=True)
    dx = (wdy - c1 - xhat * c2) * rstd.unsqueeze(-1)
    dims = tuple(range(x.dim() - 1))
    dweight = (dyf * xhat).sum(dim=dims)
    dbias = dyf.sum(dim=dims)
    return dx.to(x.dtype), dweight, dbias


def rms_norm_fwd(x: torch.Tensor, weight: torch.Tensor,
                 eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = _up(x)
    rstd = torch.rsqrt(xf.pow(2).mean(dim=-1) + eps)
    y = xf * rstd.unsqueeze(-1) * _up(weight)
    return y.to(x.dtype), rstd


def rms_norm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
                 rstd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = _up(x)
    dyf = _up(dy)
    xhat = xf * rstd.unsqueeze(-1)
    wdy = dyf * _up(weight)
    H = x.shape[-1]
    c = (wdy * xhat).mean(dim=-1, keepdim=True)
    dx = (wdy - xhat * c) * rstd.unsqueeze(-1)
    dims = tuple(range(x.dim() - 1))
    dweight = (dyf * xhat).sum(dim=dims)
    return dx.to(x.dtype), dweight


def gelu(x: torch.Tensor) -> torch.Tensor:
    # tanh approximation — matches the HIP kernel exactly
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 *
                                       (x + 0.044715 * x * x * x)))


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    k = 0.7978845608028654
    x3 = x * x * x
    t = torch.tanh(k * (x + 0.044715 * x3))
    dt = (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * x * x)
    return 0.5 * (1.0 + t) + 0.5 * x * dt


def bias_gelu_fwd(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return gelu((_up(x) + _up(bias))).to(x.dtype)


def bias_gelu_bwd(dy: torch.Tensor, x: torch.Tensor, bias: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    z = _up(x) + _up(bias)
    dx = _up(dy) * gelu_grad(z)
    dims = tuple(range(x.dim() - 1))
    dbias = dx.sum(dim=dims)
    return dx.to(x.dtype), dbias


def _fp8_dual(y: torch.Tensor, scale: torch.Tensor):
    """Delayed-scale e4m3 cast of the rounded activation y [.., F]:
    (q [N, F], qt [F, N], amax fp32 [1]) — what the dual quantize kernel
    returns for y.reshape(-1, F)."""
    y2 = y.reshape(-1, y.shape[-1])
    q = (y2.float() / scale.float().reshape(())).clamp(-448.0, 448.0).to(
        torch.float8_e4m3fn)
    if y2.numel():
        amax = y2.float().abs().amax().reshape(1)
    else:
        amax = torch.zeros(1, dtype=torch.float32, device=y.device)
    return q, q.t().contiguous(), amax


def bias_gelu_fp8(x: torch.Tensor, bias: torch.Tensor, scale: torch.Tensor):
    """gelu(x + bias) rounded to x.dtype, then cast: (q, qt, amax)."""
    return _fp8_dual(bias_gelu_fwd(x, bias), scale)


def add_layer_norm_fp8(a: torch.Tensor, delta, weight: torch.Tensor,
                       bias: torch.Tensor, eps: float, scale: torch.Tensor):
    """h = a (+ delta); y = LN(h) rounded to a.dtype, then cast:
    (h, mean, rstd, q, qt, amax)."""
    h = a + delta if delta is not None else a.clone()
    y, mean, rstd = layer_norm_fwd(h, weight, bias, eps)
    q, qt, amax = _fp8_dual(y, scale)
    return h, mean.reshape(-1), rstd.reshape(-1), q, qt, amax


def _alibi_bias(alibi, Hh, S, Skv, device):
    """[1, Hh, S, Skv] ALiBi bias: slope_h * (kv_pos - q_pos); q global
    position is offset by Skv - S (cached decode)."""
    qpos = torch.arange(S, device=device, dtype=torch.float32) + (Skv - S)
    kpos = torch.arange(Skv, device=device, dtype=torch.float32)
    rel = kpos.view(1, 1, 1, Skv) - qpos.view(1, 1, S, 1)
    return alibi.float().view(1, Hh, 1, 1) * rel


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  causal: bool = True, softmax_scale: float | None = None,
                  alibi: torch.Tensor | None = None,
                  kv_lens: torch.Tensor | None = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """q,k,v: [B, Hh, S, D]. Returns (o, lse[B,Hh,S]) in fp32 math.
    alibi: optional per-head slopes [Hh] (BLOOM bias).
    kv_lens: optional int [B] per-batch real KV lengths (varlen decode:
    positions >= kv_lens[b] are masked; alibi q position offsets per
    batch)."""
    B, Hh, S, D = q.shape
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    s = torch.matmul(_up(q), _up(k).transpose(-1, -2)) * scale
    Skv = k.shape[2]
    if alibi is not None:
        if kv_lens is not None:
            kpos = torch.arange(Skv, device=q.device, dtype=torch.float32)
            qpos = (kv_lens.to(q.device).float().view(B, 1, 1, 1) - S +
                    torch.arange(S, device=q.device,
                                 dtype=torch.float32).view(1, 1, S, 1))
            s = s + alibi.float().view(1, Hh, 1, 1) * (
                kpos.view(1, 1, 1, Skv) - qpos)
        else:
            s = s + _alibi_bias(alibi, Hh, S, Skv, q.device)
    if kv_lens is not None:
        mask = torch.arange(Skv, device=q.device).view(1, 1, 1, Skv) >=             kv_lens.to(q.device).view(B, 1, 1, 1)
        s = s.masked_fill(mask, float("-inf"))
    if causal:
        mask = torch.triu(torch.ones(S, k.shape[2], dtype=torch.bool,
                                     device=q.device), diagonal=1)
        s = s.masked_fill(mask, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    # a row with no visible key (kv_lens[b] == 0): o = 0, lse = -inf, as
    # the kernel gives; every other row has l >= 1 and is unchanged
    p = torch.exp(s - m.masked_fill(m == float("-inf"), 0.0))
    l = p.sum(dim=-1, keepdim=True)
    o = torch.matmul(p / l.masked_fill(l == 0, 1.0), _up(v))
    lse = (m + torch.log(l)).squeeze(-1)
    return o.to(q.dtype), lse


# e4m3 KV cache (csrc/kv_cache_fp8.hip, csrc/attention_decode_fp8.hip).  These
# functions are the specification the two kernels are tested against.
E4M3_MAX = 448.0


def kv_quantize_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., d] -> (bytes [..., d] float8_e4m3fn, scale [...] fp32), every
    row on its own: scale = amax(|x|) / 448 and bytes = e4m3_rne(x / scale),
    both divisions in fp32, the conversion saturating at +-448.  An all-zero
    row has scale = 1.  A row that holds a NaN or an Inf has scale = NaN and
    the e4m3 NaN code 0x7F in every byte, so the whole row dequantizes to
    NaN: nothing is clamped into range silently."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    bad = ~torch.isfinite(amax)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / E4M3_MAX)
    scale = scale.masked_fill(bad, float("nan"))
    safe = scale.masked_fill(bad, 1.0).unsqueeze(-1)
    y = (xf.masked_fill(bad.unsqueeze(-1), 0.0) / safe).clamp(-E4M3_MAX,
                                                              E4M3_MAX)
    q = y.to(torch.float8_e4m3fn)
    q.view(torch.uint8).masked_fill_(bad.unsqueeze(-1), 0x7F)
    return q, scale


def kv_dequantize_rows(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The fp32 rows that (bytes, scale) of kv_quantize_rows stand for."""
    return q.float() * scale.float().unsqueeze(-1)


def kv_cache_append_fp8(k, v, k8, k_scale, v8, v_scale, pos) -> None:
    """Quantize k, v [B, h, S, d] per row and write row (b, h, s) at cache
    position pos_b + s, in place; pos an int or an int tensor [B].  A row
    whose position is outside [0, max_len) is skipped."""
    B, _, S, _ = k.shape
    max_len = k8.shape[2]
    if not torch.is_tensor(pos):
        pos = torch.full((B,), int(pos), dtype=torch.long, device=k.device)
    at = pos.long().view(B, 1) + torch.arange(S, device=k.device).view(1, S)
    b_idx, s_idx = torch.nonzero((at >= 0) & (at < max_len), as_tuple=True)
    at = at[b_idx, s_idx]
    for x, c8, cs in ((k, k8, k_scale), (v, v8, v_scale)):
        q, sc = kv_quantize_rows(x)
        c8.view(torch.uint8)[b_idx, :, at] = q.view(torch.uint8)[b_idx, :,
                                                                 s_idx]
        cs[b_idx, :, at] = sc[b_idx, :, s_idx]


def qkv_cache_write(qkv, cache_k, cache_v, pos, rotary=None, want_k=False):
    """The specification of csrc/qkv_cache_write.hip.  qkv [B, S, h, 3, d]
    (any float dtype); cache_k, cache_v tensors [B, h, L, d] or the (bytes,
    scales) pairs of the e4m3 cache; pos an int or an int tensor [B]; rotary
    None or (sin, cos, rotary_dim) with tables [T, rotary_dim/2].  Row
    (b, head, s) sits at p = pos_b + s.  q and k are rotated (GPT-J
    interleaved pairs, the first rotary_dim columns) in fp32, every multiply,
    add and subtract rounded on its own, and rounded to qkv's dtype; k and v
    go to cache row p (an e4m3 cache through kv_cache_append_fp8 of the
    rounded rows).  A row with p outside [0, L), or outside the tables, is
    zero in q (and k_new) and writes nothing.  Returns q [B, h, S, d]
    contiguous, or (q, k_new) with want_k."""
    B, S, h, _, d = qkv.shape
    dev = qkv.device
    fp8 = isinstance(cache_k, tuple)
    L = (cache_k[0] if fp8 else cache_k).shape[2]
    if torch.is_tensor(pos):
        p0 = pos.to(dev).long()
    else:
        p0 = torch.full((B,), int(pos), dtype=torch.long, device=dev)
    at = p0.view(B, 1) + torch.arange(S, device=dev).view(1, S)
    q, k, v = (qkv[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))
    if rotary is not None:
        sin, cos, rd = rotary
        T = sin.shape[0]
        if not torch.is_tensor(pos) and not 0 <= int(pos) <= T - S:
            raise ValueError(f"positions {pos} .. {int(pos) + S - 1} are "
                             f"outside the rotary tables of {T} rows")
        L = min(L, T)
        row = at.clamp(0, max(T - 1, 0))
        sn = sin.to(dev).float()[row].view(B, 1, S, rd // 2)
        cs = cos.to(dev).float()[row].view(B, 1, S, rd // 2)

        def rot(x):
            pairs = x[..., :rd].float().reshape(B, h, S, rd // 2, 2)
            x0, x1 = pairs[..., 0], pairs[..., 1]
            y = torch.stack([x0 * cs - x1 * sn, x0 * sn + x1 * cs], dim=-1)
            return torch.cat([y.flatten(-2).to(x.dtype), x[..., rd:]], dim=-1)

        q, k = rot(q), rot(k)
    valid = (at >= 0) & (at < L)
    keep = valid.view(B, 1, S, 1)
    q_out = torch.where(keep, q, torch.zeros_like(q)).contiguous()
    k_new = torch.where(keep, k, torch.zeros_like(k)).contiguous()
    # rows at or past min(L, T) are skipped: write through views that end there
    if fp8:
        (k8, ks), (v8, vs) = cache_k, cache_v
        kv_cache_append_fp8(k, v, k8[:, :, :L], ks[:, :, :L], v8[:, :, :L],
                            vs[:, :, :L], p0)
    else:
        b_idx, s_idx = torch.nonzero(valid, as_tuple=True)
        rows = at[b_idx, s_idx]
        cache_k[b_idx, :, rows] = k[b_idx, :, s_idx].to(cache_k.dtype)
        cache_v[b_idx, :, rows] = v[b_idx, :, s_idx].to(cache_v.dtype)
    return (q_out, k_new) if want_k else q_out


def attention_decode_fp8(q, k8, k_scale, v8, v_scale, softmax_scale=None,
                         alibi=None, kv_lens=None):
    """attention_fwd (non-causal) over the dequantized cache; rows at or
    past a slot's length are never looked at, whatever they hold."""
    k = kv_dequantize_rows(k8, k_scale)
    v = kv_dequantize_rows(v8, v_scale)
    if kv_lens is not None:
        dead = (torch.arange(k.shape[2], device=k.device).view(1, 1, -1, 1)
                >= kv_lens.to(k.device).view(-1, 1, 1, 1))
        k, v = k.masked_fill(dead, 0.0), v.masked_fill(dead, 0.0)
    return attention_fwd(q, k, v, False, softmax_scale, alibi, kv_lens)


def attention_chunk(q, k, v, softmax_scale=None, alibi=None, kv_lens=None):
    """Sq query rows over a cache that already holds them: q [B, Hh, Sq, D],
    k, v [B, Hh, Skv, D], len_b = kv_lens[b] clamped to [0, Skv] (Skv without
    lengths).  Row i of slot b sits at position p = len_b - Sq + i and sees
    keys j <= p (a causal mask aligned bottom-right); ALiBi adds
    slope * (j - p).  A row with p < 0 gives o = 0, lse = -inf.  Rows of k
    and v at or past len_b are never looked at.  Returns (o, lse [B,Hh,Sq])
    in fp32 math."""
    B, Hh, Sq, D = q.shape
    Skv = k.shape[2]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    if kv_lens is None:
        lens = torch.full((B,), Skv, dtype=torch.long, device=q.device)
    else:
        lens = kv_lens.to(q.device).long().clamp(0, Skv)
    kpos = torch.arange(Skv, device=q.device).view(1, 1, 1, Skv)
    pos = lens.view(B, 1, 1, 1) - Sq + \
        torch.arange(Sq, device=q.device).view(1, 1, Sq, 1)
    dead = (kpos >= lens.view(B, 1, 1, 1)).view(B, 1, Skv, 1)
    kf, vf = _up(k).masked_fill(dead, 0.0), _up(v).masked_fill(dead, 0.0)
    s = torch.matmul(_up(q), kf.transpose(-1, -2)) * scale
    if alibi is not None:
        s = s + alibi.float().view(1, Hh, 1, 1) * (kpos - pos).float()
    s = s.masked_fill(kpos > pos, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m.masked_fill(m == float("-inf"), 0.0))
    l = p.sum(dim=-1, keepdim=True)
    o = torch.matmul(p / l.masked_fill(l == 0, 1.0), vf)
    lse = (m + torch.log(l)).squeeze(-1)
    return o.to(q.dtype), lse


def attention_chunk_fp8(q, k8, k_scale, v8, v_scale, softmax_scale=None,
                        alibi=None, kv_lens=None):
    """attention_chunk over the dequantized cache."""
    return attention_chunk(q, kv_dequantize_rows(k8, k_scale),
                           kv_dequantize_rows(v8, v_scale), softmax_scale,
                           alibi, kv_lens)


def attention_bwd(do: torch.Tensor, q: torch.Tensor, k: torch.Tensor,
                  v: torch.Tensor, o: torch.Tensor, lse: torch.Tensor,
                  causal: bool = True, softmax_scale: float | None = None,
                  alibi: torch.Tensor | None = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    B, Hh, S, D = q.shape
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf, dof = _up(q), _up(k), _up(v), _up(do)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if alibi is not None:
        s = s + _alibi_bias(alibi, Hh, S, k.shape[2], q.device)
    if causal:
        mask = torch.triu(torch.ones(S, k.shape[2], dtype=torch.bool,
                                     device=q.device), diagonal=1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1))
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * _up(o)).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def softmax_cross_entropy_fwd(logits: torch.Tensor, targets: torch.Tensor
                              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [N, V], targets [N] int64. Returns (loss[N], lse[N])."""
    lf = _up(logits)
    lse = torch.logsumexp(lf, dim=-1)
    loss = lse - lf.gather(-1, targets.unsqueeze(-1)).squeeze(-1)
    return loss, lse


def softmax_cross_entropy_bwd(dloss: torch.Tensor, logits: torch.Tensor,
                              targets: torch.Tensor, lse: torch.Tensor
                              ) -> torch.Tensor:
    p = torch.exp(_up(logits) - lse.unsqueeze(-1))
    p.scatter_add_(-1, targets.unsqueeze(-1),
                   -torch.ones_like(targets, dtype=p.dtype).unsqueeze(-1))
    return (p * _up(dloss).unsqueeze(-1)).to(logits.dtype)


def _shard_target(targets: torch.Tensor, vocab_start: int, width: int):
    """(owned [N] bool, column [N]) of global target ids inside the vocab
    shard [vocab_start, vocab_start + width); the column of a target the
    shard does not own is clamped into range and must not be used."""
    local = targets - vocab_start
    owned = (local >= 0) & (local < width)
    return owned, local.clamp(0, width - 1)


def softmax_cross_entropy_partial(logits: torch.Tensor, targets: torch.Tensor,
                                  vocab_start: int) -> torch.Tensor:
    """Combinable row statistics of one vocab shard: logits [N, Vs] holds
    global columns [vocab_start, vocab_start + Vs), targets [N] are global
    ids.  Returns stats [3, N]: the shard's row max m (-inf for a row of
    -inf only), s = sum exp(x - m) (0 where m = -inf) and t = the target
    logit where the shard owns the target, else 0."""
    lf = _up(logits)
    m = lf.max(dim=-1).values
    # a fully masked row: shift by 0, every exp(-inf) is 0
    shift = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    s = torch.exp(lf - shift.unsqueeze(-1)).sum(dim=-1)
    owned, col = _shard_target(targets, vocab_start, lf.shape[-1])
    t = lf.gather(-1, col.unsqueeze(-1)).squeeze(-1)
    t = torch.where(owned, t, torch.zeros_like(t))
    return torch.stack([m, s, t])


def softmax_cross_entropy_combine(stats: torch.Tensor
                                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """stats [T, 3, N], the partial statistics of T vocab shards in rank
    order -> (loss [N], lse [N]) over the whole vocab.  The sums run in
    rank order, so every rank that holds the same stats gets the same
    bits.  A shard with m = -inf adds nothing; a row masked on every shard
    is undefined."""
    m, s, t = stats[:, 0], stats[:, 1], stats[:, 2]
    gm = m.max(dim=0).values
    # s = 0 wherever m = -inf, and exp(-inf - gm) = 0: the product is 0
    w = s * torch.exp(m - gm)
    gs, gt = w[0], t[0]
    for r in range(1, stats.shape[0]):
        gs = gs + w[r]
        gt = gt + t[r]
    lse = gm + torch.log(gs)
    return lse - gt, lse


def softmax_cross_entropy_shard_bwd(dloss: torch.Tensor, logits: torch.Tensor,
                                    targets: torch.Tensor, lse: torch.Tensor,
                                    vocab_start: int) -> torch.Tensor:
    """dlogits of one vocab shard from the whole-vocab lse: (exp(x - lse) -
    onehot) * dloss, the one-hot only where the shard owns the target."""
    p = torch.exp(_up(logits) - lse.unsqueeze(-1))
    owned, col = _shard_target(targets, vocab_start, logits.shape[-1])
    p.scatter_add_(-1, col.unsqueeze(-1), -owned.to(p.dtype).unsqueeze(-1))
    return (p * _up(dloss).unsqueeze(-1)).to(logits.dtype)


def logits_topk(logits: torch.Tensor, k: int, inv_temperature=None,
                vocab_start: int = 0):
    """Top-k of y = float(logits) * inv_temperature[b] (one fp32 multiply)
    with the statistics of a softmax over the row: (vals [B, k] fp32 sorted
    descending, equal y by lower column; idx [B, k] int64 = column +
    vocab_start; m [B] = max y; s [B] = sum exp(y - m), summed in fp64, 0
    for a row of -inf only).  k is clamped to V.  A NaN in a row makes its
    m and s NaN."""
    B, V = logits.shape
    y = logits.float()
    if inv_temperature is not None:
        y = y * inv_temperature.float().reshape(B, 1)
    # a stable sort keeps equal values in column order
    vals, idx = torch.sort(y, dim=-1, descending=True, stable=True)
    k = min(int(k), V)
    m = y.max(dim=-1).values
    shift = torch.where(m == -math.inf, torch.zeros_like(m), m).double()
    s = torch.exp(y.double() - shift.unsqueeze(-1)).sum(dim=-1)
    return (vals[:, :k].contiguous(), idx[:, :k] + int(vocab_start), m,
            s.float())


def sample_logits(logits: torch.Tensor, u: torch.Tensor,
                  inv_temperature: torch.Tensor, top_k: torch.Tensor,
                  top_p: torch.Tensor, k: int = 64) -> torch.Tensor:
    """One token per row by temperature / top-k / top-p sampling with an
    inverse-CDF draw, every parameter per row ([B] tensors).  Over the first
    n = (top_k if 0 < top_k <= k else k) entries of logits_topk(logits, k,
    inv_temperature): p_j = exp(y_j - y_0), e_j = sum of p_i for i < j, T
    their total; candidate j is kept iff j == 0 or e_j < top_p * T; T' is
    the kept sum; the token is the first kept j with e_j + p_j > u * T',
    else the last kept one.  A row whose y_0 is -inf or NaN gives candidate
    0.  Arithmetic after y in fp64."""
    vals, idx, _, _ = logits_topk(logits, k, inv_temperature)
    kk = vals.shape[1]
    j = torch.arange(kk, device=vals.device).unsqueeze(0)
    tk = top_k.long().reshape(-1, 1)
    n = torch.where((tk > 0) & (tk <= kk), tk, torch.full_like(tk, kk))
    y = vals.double()
    p = torch.where(j < n, torch.exp(y - y[:, :1]), torch.zeros_like(y))
    e = p.cumsum(dim=-1) - p
    T = p.sum(dim=-1, keepdim=True)
    keep = (j < n) & ((j == 0) | (e < top_p.double().reshape(-1, 1) * T))
    kept_sum = (p * keep).sum(dim=-1, keepdim=True)
    hit = keep & (e + p > u.double().reshape(-1, 1) * kept_sum)
    pick = torch.where(hit.any(dim=-1), hit.int().argmax(dim=-1),
                       keep.sum(dim=-1) - 1)
    pick = torch.where(vals[:, 0] > -math.inf, pick, torch.zeros_like(pick))
    return idx.gather(1, pick.unsqueeze(1))[:, 0]


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, step: int, lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float,
               grad_scale: float = 1.0, grad_sumsq=None,
               max_grad_norm=None, twins=None):
    """In-place multi-tensor AdamW (fp32 master math on fp32 state).

    twins, aligned with params, holds None or a [cols, rows] tensor that
    receives the transpose of the updated [rows, cols] parameter.

    With grad_sumsq (a one-element tensor, the sum of squares of all raw
    gradients) and max_grad_norm, the gradients are clipped by global norm
    as optax.clip_by_global_norm does: scaled by grad_scale * max_grad_norm
    / max(norm, max_grad_norm), norm = |grad_scale| * sqrt(grad_sumsq).
    The clip math runs in grad_sumsq's dtype.  A non-finite norm leaves
    params and moments as they were; like the kernel, this is decided by
    torch.where on tensors and never by a host branch on tensor data."""
    if (grad_sumsq is None) != (max_grad_norm is None):
        raise ValueError(
            "grad_sumsq and max_grad_norm must be given together")
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    if grad_sumsq is None:
        for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
            gf = _up(g) * grad_scale
            pf = _up(p)
            pf.mul_(1.0 - lr * weight_decay)
            m.mul_(beta1).add_(gf, alpha=1.0 - beta1)
            v.mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
            denom = (v / bc2).sqrt_().add_(eps)
            pf.addcdiv_(m / bc1, denom, value=-lr)
            p.copy_(pf.to(p.dtype))
        _write_twins(params, twins)
        return
    if not max_grad_norm > 0:
        raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
    norm = abs(grad_scale) * _up(grad_sumsq).reshape(()).sqrt()
    ok = torch.isfinite(norm)
    limit = torch.full_like(norm, max_grad_norm)
    scale = grad_scale * (limit / torch.maximum(norm, limit))
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        gf = _up(g) * scale.to(m.dtype)
        # the unclipped update above, op for op, on copies
        pf = _up(p).clone().mul_(1.0 - lr * weight_decay)
        m_new = m.clone().mul_(beta1).add_(gf, alpha=1.0 - beta1)
        v_new = v.clone().mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
        denom = (v_new / bc2).sqrt_().add_(eps)
        pf.addcdiv_(m_new / bc1, denom, value=-lr)
        m.copy_(torch.where(ok, m_new, m))
        v.copy_(torch.where(ok, v_new, v))
        p.copy_(torch.where(ok, pf.to(p.dtype), p))
    # p is unchanged on a non-finite norm, and then so is its transpose
    _write_twins(params, twins)


def _write_twins(params, twins):
    for p, t in zip(params, twins or ()):
        if t is not None:
            t.copy_(p.t())


def multi_tensor_sumsq(tensors) -> torch.Tensor:
    """Sum of squares over all elements of all tensors, shape [1]: fp32
    (half precision is upcast), or fp64 if the tensors are."""
    total = None
    for t in tensors:
        tf = _up(t).reshape(-1)
        s = (tf * tf).sum()
        total = s if total is None else total + s
    return total.reshape(1)


# ------------------------------ MoE routing --------------------------------
# Fixed-shape, sync-free top-2 routing: no boolean indexing, no nonzero.
# Integer outputs are int32, like the HIP kernels'.

def _moe_top2_indices(lf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """idx1 = argmax, idx2 = argmax over the rest; the lowest index wins a
    tie, stated explicitly rather than left to topk/argmax.

    A NaN never wins a comparison: it counts as below everything, except
    that a NaN in the column a scan would start from (column 0 for idx1,
    the lowest column != idx1 for idx2) is never displaced.  This is what
    a left-to-right scan with a strict '>' gives, and it keeps
    0 <= idx1 != idx2 < E for any row."""
    N, E = lf.shape
    ar = torch.arange(E, device=lf.device).expand(N, E)
    nan = torch.isnan(lf)
    ninf = torch.full_like(lf, float("-inf"))
    pinf = torch.full_like(lf, float("inf"))
    key = torch.where(nan, ninf, lf)
    key1 = torch.where(nan & (ar == 0), pinf, key)
    m1 = key1.max(dim=-1, keepdim=True).values
    idx1 = torch.where(key1 == m1, ar, E).min(dim=-1).values
    first = ar == idx1.unsqueeze(-1)
    j0 = (idx1 == 0).long().unsqueeze(-1)
    key2 = torch.where(nan & (ar == j0), pinf, key)
    m2 = torch.where(first, ninf, key2).max(dim=-1, keepdim=True).values
    idx2 = torch.where((key2 == m2) & ~first, ar, E).min(dim=-1).values
    return idx1, idx2


def moe_top2_route(logits: torch.Tensor, capacity: int):
    """Top-2 gate with capacity slots.  logits [N, E] ->
    (w1, w2, idx1, idx2, slot1, slot2, src, aux, count1).

    p = softmax(logits); w_k = p_k / (p1 + p2), normalised before drops;
    pos1[t] counts earlier tokens with the same first choice, pos2[t]
    starts behind min(count1, C); slot_k = idx_k * C + pos_k, or -1 when
    pos_k >= C; src[s] is the token in slot s or -1;
    aux = E * sum_e mean_t(p[t, e]) * count1[e] / N.  Written in
    differentiable torch ops, so autograd through w1, w2 and aux works."""
    lf = _up(logits)
    N, E = lf.shape
    C = int(capacity)
    p = torch.softmax(lf, dim=-1)
    idx1, idx2 = _moe_top2_indices(lf.detach())
    p1 = p.gather(1, idx1.unsqueeze(-1)).squeeze(-1)
    p2 = p.gather(1, idx2.unsqueeze(-1)).squeeze(-1)
    den = p1 + p2
    w1, w2 = p1 / den, p2 / den

    ar = torch.arange(E, device=lf.device)
    oh1 = (idx1.unsqueeze(-1) == ar).long()
    oh2 = (idx2.unsqueeze(-1) == ar).long()
    count1 = oh1.sum(0)
    pos1 = ((oh1.cumsum(0) - oh1) * oh1).sum(-1)
    pos2 = ((oh2.cumsum(0) - oh2 + count1.clamp(max=C)) * oh2).sum(-1)
    none = torch.full_like(pos1, -1)
    slot1 = torch.where(pos1 < C, idx1 * C + pos1, none)
    slot2 = torch.where(pos2 < C, idx2 * C + pos2, none)
    # dropped choices land in one spare entry past the end
    t = torch.arange(N, device=lf.device)
    spare = torch.full_like(pos1, E * C)
    src = torch.full((E * C + 1,), -1, dtype=torch.long, device=lf.device)
    src.scatter_(0, torch.where(slot1 >= 0, slot1, spare), t)
    src.scatter_(0, torch.where(slot2 >= 0, slot2, spare), t)
    src = src[:E * C]
    if N > 0:
        aux = E * (p.mean(dim=0) * (count1.to(p.dtype) / N)).sum()
    else:
        aux = p.new_zeros(())
    i32 = torch.int32
    return (w1, w2, idx1.to(i32), idx2.to(i32), slot1.to(i32),
            slot2.to(i32), src.to(i32), aux, count1.to(i32))


def moe_top2_route_bwd(logits, idx1, idx2, w1, w2, count1, dw1, dw2, daux):
    """dlogits of (w1, w2, aux); count1 is a constant.
    d aux / d p[t, e] = E * count1[e] / N^2, through the softmax;
    dl1 = (dw1 - dw2) * w1 * w2 = -dl2 on the two chosen columns."""
    lf = _up(logits)
    N, E = lf.shape
    p = torch.softmax(lf, dim=-1)
    dp = (daux.to(p.dtype) * E / (N * N)) * count1.to(p.dtype)
    dl = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
    dl1 = ((dw1 - dw2) * w1 * w2).to(p.dtype).unsqueeze(-1)
    dl = dl.scatter_add(1, idx1.long().unsqueeze(-1), dl1)
    dl = dl.scatter_add(1, idx2.long().unsqueeze(-1), -dl1)
    return dl.to(logits.dtype)


def _moe_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x[idx] with zero rows where idx < 0 (fixed shape)."""
    if x.shape[0] == 0:
        return x.new_zeros(idx.shape[0], x.shape[1])
    rows = x.index_select(0, idx.clamp_min(0).long())
    return torch.where((idx >= 0).unsqueeze(-1), rows, torch.zeros_like(rows))


def moe_dispatch(x: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """x [N, H], src [E*C] -> [E*C, H]: row s is x[src[s]], zeros if empty."""
    return _moe_rows(x, src)


def moe_combine(y: torch.Tensor, w1, w2, slot1: torch.Tensor,
                slot2: torch.Tensor) -> torch.Tensor:
    """out[t] = w1[t] * y[slot1[t]] + w2[t] * y[slot2[t]], dropped terms
    skipped; summed in the upcast dtype and rounded once.  w1 = w2 = None
    means unit weights, which makes this the backward of moe_dispatch."""
    yf = _up(y)
    a, b = _moe_rows(yf, slot1), _moe_rows(yf, slot2)
    if w1 is not None:
        # where, not a bare product: a dropped choice of a NaN-weighted
        # token must contribute nothing
        a = torch.where((slot1 >= 0).unsqueeze(-1),
                        w1.to(yf.dtype).unsqueeze(-1) * a, a)
        b = torch.where((slot2 >= 0).unsqueeze(-1),
                        w2.to(yf.dtype).unsqueeze(-1) * b, b)
    return (a + b).to(y.dtype)


def moe_dispatch_bwd(g: torch.Tensor, slot1: torch.Tensor,
                     slot2: torch.Tensor) -> torch.Tensor:
    """dx[t] = g[slot1[t]] + g[slot2[t]]."""
    return moe_combine(g, None, None, slot1, slot2)


def moe_combine_bwd(dout: torch.Tensor, y: torch.Tensor, w1: torch.Tensor,
                    w2: torch.Tensor, slot1: torch.Tensor,
                    slot2: torch.Tensor, src: torch.Tensor):
    """(dy, dw1, dw2): dy[s] = w_k * dout[src[s]] with k the choice that
    owns slot s; dw_k[t] = <dout[t], y[slot_k[t]]>, 0 when dropped."""
    df, yf = _up(dout), _up(y)
    S = src.shape[0]
    tok = src.clamp_min(0).long()
    if dout.shape[0] == 0:
        dy = torch.zeros_like(y)
    else:
        first = slot1.index_select(0, tok) == torch.arange(S,
                                                           device=src.device)
        scale = torch.where(first, w1.index_select(0, tok),
                            w2.index_select(0, tok)).to(df.dtype)
        rows = scale.unsqueeze(-1) * df.index_select(0, tok)
        dy = torch.where((src >= 0).unsqueeze(-1), rows,
                         torch.zeros_like(rows)).to(y.dtype)
    dw1 = (df * _moe_rows(yf, slot1)).sum(-1).to(w1.dtype)
    dw2 = (df * _moe_rows(yf, slot2)).sum(-1).to(w2.dtype)
    return dy, dw1, dw2


# ------------------- MXFP4 weights (OCP microscaling) ------------------------
# e2m1 codes sign<<3 | exp<<1 | mant and one e8m0 scale byte per 32 k.  These
# functions are the format's specification; ops.mxfp4_quantize and
# ops.mxfp4_dequantize are these, and skinny_linear_fp4 is the oracle of the
# two MXFP4 kernels.
#: the 8 magnitudes of e2m1, by code & 7
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mxfp4_quantize(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K], K % 32 == 0 -> (codes uint8 [N, K/2], scales uint8
    [N, K/32]).  Per block of 32 along K: E = clamp(floor(log2(amax)) - 2 +
    127, 2, 252), which keeps every dequantized value a normal bf16 (127 for
    a block of zeros); each element x / 2^(E-127), an exact fp32 product, is
    rounded to the nearest e2m1 value, ties to the even code, saturating at
    +-6.  The even k goes in the low nibble.  Only integer and exact fp32
    steps, so every device gives the same bytes.  ValueError on a non-finite
    weight."""
    N, K = w.shape
    if K % 32:
        raise ValueError(f"mxfp4_quantize: K must be a multiple of 32, got {K}")
    xf = w.detach().float().reshape(N, K // 32, 32)
    if not bool(torch.isfinite(xf).all()):
        raise ValueError("mxfp4_quantize: the weight holds a NaN or an Inf")
    amax = xf.abs().amax(dim=-1)
    # floor(log2(amax)) + 127 is the fp32 exponent field (0 for subnormals,
    # which the clamp covers)
    field = (amax.view(torch.int32) >> 23) & 0xFF
    E = torch.where(amax == 0, torch.full_like(field, 127),
                    (field - 2).clamp(2, 252))
    inv = ((254 - E) << 23).view(torch.float32)  # 2^(127-E)
    a = (xf * inv.unsqueeze(-1)).abs()
    # one step per midpoint; >= where the tie goes up to the even code
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25)
            + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code = (code | (torch.signbit(xf).to(torch.uint8) << 3)).reshape(N, K)
    codes = code[:, 0::2] | (code[:, 1::2] << 4)
    return codes.contiguous(), E.to(torch.uint8)


def mxfp4_dequantize(codes: torch.Tensor, scales: torch.Tensor,
                     dtype=torch.bfloat16) -> torch.Tensor:
    """The [N, K] weights that (codes, scales) stand for: e2m1 value times
    2^(E-127), exact in fp32 and, for 2 <= E <= 252, in bf16."""
    N, K = codes.shape[0], codes.shape[1] * 2
    nib = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(N, K).long()
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES),
                       dtype=torch.float32, device=codes.device)
    E = scales.to(torch.int32)
    # 2^(E-127) from the exponent field; E = 0 is the fp32 subnormal 2^-127
    factor = torch.where(E == 0, torch.full_like(E, 0x00400000),
                         E << 23).view(torch.float32)
    val = lut[nib].reshape(N, K // 32, 32) * factor.unsqueeze(-1)
    return val.reshape(N, K).to(dtype)


def skinny_linear_fp4(x: torch.Tensor, codes: torch.Tensor,
                      scales: torch.Tensor, bias=None) -> torch.Tensor:
    """y = x @ dequantize(codes, scales)^T (+ bias): fp32 matmul on the exact
    weights, rounded once to x's dtype."""
    w = mxfp4_dequantize(codes, scales, torch.float32)
    y = x.float().reshape(-1, w.shape[1]) @ w.t()
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype).reshape(*x.shape[:-1], w.shape[0])
