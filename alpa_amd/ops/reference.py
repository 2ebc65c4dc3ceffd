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


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, step: int, lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float,
               grad_scale: float = 1.0, grad_sumsq=None,
               max_grad_norm=None):
    """In-place multi-tensor AdamW (fp32 master math on fp32 state).

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
