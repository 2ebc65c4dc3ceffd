"""Shared by test_attention_fwd_exact_gpu.py and
test_attention_fwd_cases_cpu.py: input builders for the attention forward
kernel with the outputs they must produce, an fp64 reference with the
derived error bound, and a plain emulation of the kernel's tile loop.

Every builder works on the CPU in bf16 and returns a `Case`; the GPU tests
move the tensors to the device.  Expected values of the exact families come
from the construction, not from a softmax."""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

B, H = 2, 2
TILE = 64        # kv per tile of the kernel
WAVE_ROWS = 16   # q rows per wave
DEFER_THR = 8.0  # the kernel's deferred-rescale threshold

A_SCALE = 64.0
B_SCALE = 0.5
C_SCALE = 0.125
LSE_ATOL = 1e-3  # families C and D; A and B carry the sharp lse checks

# (S, Skv, D, causal).  Every head-dim tile with D strictly inside it
# (16, 48 | 80 | 112 | 160) and filling it (64, 96, 128, 256); ragged S and
# Skv around the 16-row wave and the 64-wide tile; one and two blocks of
# 128 q rows; causal with Skv > S and with Skv < S.
AB_SHAPES = [
    (130, 200, 16, False),
    (200, 200, 64, True),
    (67, 256, 96, False),
    (192, 192, 256, True),
    (1, 1, 48, False),
    (16, 63, 80, False),
    (1, 64, 112, False),
    (16, 65, 128, True),
    (130, 64, 160, True),
    (192, 65, 112, True),
    (67, 200, 48, True),
    (200, 256, 80, False),
]
# Skv = 257 has no distinct 8-bit codes: families B, C and D only
B_ONLY_SHAPES = [
    (130, 257, 96, False),
    (1, 257, 16, False),
]
# (S, Skv, D, kv_lens): lengths 1, 64, 65 and Skv, and empty slots
VARLEN_SHAPES = [
    (1, 200, 64, (1, 200)),
    (16, 200, 80, (64, 0)),
    (16, 256, 128, (65, 256)),
    (1, 65, 48, (0, 65)),
    (130, 200, 112, (200, 64)),
]
B_ONLY_VARLEN_SHAPES = [
    (1, 257, 64, (257, 65)),
]
# family B varlen cases whose tail is poisoned: a tail that starts on a tile
# edge with an empty slot, and one that starts inside a tile
TAIL_SHAPES = [
    (16, 200, 80, (64, 0)),
    (1, 257, 64, (257, 65)),
]
# (S, d, causal) through the packed-qkv views; d = 80 sits inside Dp = 96,
# d = 160 inside Dp = 256
VIEW_SHAPES = [
    (130, 80, True),
    (130, 160, False),
]
# (S, Skv, D, causal, order)
STAIR_SHAPES = [(200, 200, D, True, order) for D in (64, 96, 128)
                for order in ("asc", "desc", "shuffled")] + \
               [(130, 257, D, False, order) for D in (64, 96, 128)
                for order in ("asc", "desc", "shuffled")]
# (S, Skv, D, causal, alibi, kv_lens)
RANDOM_SHAPES = [
    (1, 257, 64, False, True, (100, 257)),
    (16, 130, 80, False, True, (130, 17)),
    (16, 200, 128, False, True, (65, 200)),
    (130, 130, 64, True, True, None),
    (67, 67, 96, True, False, None),
    (130, 200, 112, False, False, None),
    (1, 257, 64, False, False, None),
]


@dataclass
class Case:
    q: torch.Tensor                  # [B, H, S, D] bf16
    k: torch.Tensor                  # [B, H, Skv, D] bf16
    v: torch.Tensor
    causal: bool
    scale: float
    kv_lens: Optional[torch.Tensor] = None   # [B] int32
    alibi: Optional[torch.Tensor] = None     # [H] fp32
    o: Optional[torch.Tensor] = None         # expected, bf16 (exact families)
    lse: Optional[torch.Tensor] = None       # expected, fp32 [B, H, S]
    info: dict = field(default_factory=dict)


def _gen(*key):
    seed = 0
    for x in key:
        seed = (seed * 1000003 + int(x)) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _lens_tensor(kv_lens):
    if kv_lens is None:
        return None
    assert len(kv_lens) == B
    return torch.tensor(kv_lens, dtype=torch.int32)


def visible(S, Skv, causal, kv_lens=None):
    """[B, 1, S, Skv] bool: top-left aligned causal mask (query i sees
    kv <= i) and the per-slot length."""
    kv = torch.arange(Skv).view(1, 1, 1, Skv)
    vis = torch.ones(B, 1, S, Skv, dtype=torch.bool)
    if causal:
        vis = vis & (kv <= torch.arange(S).view(1, 1, S, 1))
    if kv_lens is not None:
        vis = vis & (kv < kv_lens.long().view(B, 1, 1, 1))
    return vis


# ---------------------------------------------------------------- family A

def one_hot_codes(Skv, D, gen):
    """[B, H, Skv, D] of +-1: columns 0..7 the bits of the row index, the
    rest random and therefore not periodic in the column."""
    assert Skv <= 256 and D >= 8
    code = (torch.randint(0, 2, (B, H, Skv, D), generator=gen) * 2 - 1)
    bits = (torch.arange(Skv).view(Skv, 1) >> torch.arange(8).view(1, 8)) & 1
    code[..., :8] = (bits * 2 - 1).view(1, 1, Skv, 8)
    return code.to(torch.bfloat16)


def one_hot(S, Skv, D, causal, kv_lens=None):
    """q[i] = k[pi(i)] with +-1 codes and scale 64: the matched score is
    64 D and every other one at least 128 lower, so in fp32 the softmax is
    exactly one-hot, o = v[pi] and lse = 64 D."""
    gen = _gen(1, S, Skv, D, causal, *(kv_lens or ()))
    lens = _lens_tensor(kv_lens)
    k = one_hot_codes(Skv, D, gen)
    v = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    vis = visible(S, Skv, causal, lens)
    n_vis = vis.sum(-1).expand(B, H, S)              # [B, H, S]
    u = torch.rand(B, H, S, generator=gen)
    # the visible keys of a row are 0..n-1
    pi = torch.minimum((u * n_vis).long(), (n_vis - 1).clamp(min=0))
    empty = n_vis == 0
    idx = pi.unsqueeze(-1).expand(B, H, S, D)
    q = k.gather(2, idx)
    o = v.gather(2, idx).clone()
    o[empty] = 0
    lse = torch.full((B, H, S), A_SCALE * D, dtype=torch.float32)
    lse[empty] = -math.inf

    # builder's own check: the gap, in fp64, on every visible pair
    s = (q.double() @ k.double().transpose(-1, -2)) * A_SCALE
    matched = torch.zeros(B, H, S, Skv, dtype=torch.bool)
    matched.scatter_(3, pi.unsqueeze(-1), True)
    live = ~empty
    assert bool((s[matched].view(B, H, S)[live] == A_SCALE * D).all())
    others = s.masked_fill(matched | ~vis.expand(B, H, S, Skv), -math.inf)
    gap = A_SCALE * D - others.max(-1).values
    assert bool((gap[live] >= 128.0).all()), "one-hot gap below 128"
    tiles = torch.unique(pi[live] // TILE).tolist()
    return Case(q, k, v, causal, A_SCALE, lens, None, o, lse,
                dict(min_gap=float(gap[live].min()), matched_tiles=tiles))


# ---------------------------------------------------------------- family B

def ternary(gen, *shape):
    return torch.randint(-1, 2, shape, generator=gen).to(torch.bfloat16)


def uniform(S, Skv, D, causal, kv_lens=None):
    """q = 0: every visible key weighs 1/n, so o = bf16(sum of the visible
    ternary v / n) with an exact integer sum, and lse = log n."""
    gen = _gen(2, S, Skv, D, causal, *(kv_lens or ()))
    lens = _lens_tensor(kv_lens)
    q = torch.zeros(B, H, S, D, dtype=torch.bfloat16)
    k = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    v = ternary(gen, B, H, Skv, D)
    vis = visible(S, Skv, causal, lens).expand(B, H, S, Skv)
    n = vis.sum(-1)                                           # [B, H, S]
    sums = vis.double() @ v.double()
    assert bool((sums == sums.round()).all()) and int(n.max()) <= 320
    o = torch.where(n.unsqueeze(-1) > 0,
                    sums / n.clamp(min=1).unsqueeze(-1).double(),
                    torch.zeros_like(sums)).to(torch.bfloat16)
    lse64 = torch.log(n.double())                             # log 0 = -inf
    return Case(q, k, v, causal, B_SCALE, lens, None, o,
                lse64.to(torch.float32), dict(n=n, lse64=lse64))


def poison_tail(case, which, value):
    """A copy of a varlen case with k or v set to `value` at and past each
    slot's length."""
    Skv = case.k.shape[2]
    tail = (torch.arange(Skv).view(1, 1, Skv, 1) >=
            case.kv_lens.long().view(B, 1, 1, 1)).expand_as(case.k)
    assert bool(tail.any())
    k, v = case.k.clone(), case.v.clone()
    (k if which == "k" else v)[tail] = value
    return Case(case.q, k, v, case.causal, case.scale, case.kv_lens,
                case.alibi, case.o, case.lse, case.info)


# ---------------------------------------------------------------- family C

def stair_levels(n_tiles, order):
    if order == "asc":
        return list(range(n_tiles))
    if order == "desc":
        return list(range(n_tiles - 1, -1, -1))
    assert order == "shuffled"
    # odd positions first, then the even ones: 1 3 0 2 4 for five tiles
    return list(range(1, n_tiles, 2)) + list(range(0, n_tiles, 2))


def staircase(S, Skv, D, causal, order):
    """Column 0 adds g_i * level(tile) to the scores: in every 16-row wave
    the row with g = 9 outruns the deferral threshold at each step up and
    forces the wave-wide rescale, and its neighbours rescale by
    alpha = exp(-g_i) in (0, 1)."""
    gen = _gen(3, S, Skv, D, causal, len(order))
    q = torch.randn(B, H, S, D, generator=gen)
    k = torch.randn(B, H, Skv, D, generator=gen) * 0.5
    v = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    i = torch.arange(S)
    g = torch.where(i % 16 == 0, torch.full((S,), 9.0), (i % 16) / 4.0)
    n_tiles = (Skv + TILE - 1) // TILE
    level = torch.tensor(stair_levels(n_tiles, order), dtype=torch.float32)
    step = level[torch.arange(Skv) // TILE] / C_SCALE
    q[..., 0] = g
    k[..., 0] = step
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    # builder's own check: the staircase survives the cast to bf16
    assert bool((q[..., 0].double() == g.double()).all())
    assert bool((k[..., 0].double() == step.double()).all())
    return Case(q, k, v, causal, C_SCALE)


# ---------------------------------------------------------------- family D

def random_case(S, Skv, D, causal, alibi, kv_lens):
    from alpa_amd.models.bloom import alibi_slopes
    gen = _gen(4, S, Skv, D, causal, alibi, *(kv_lens or ()))
    q = torch.randn(B, H, S, D, generator=gen).to(torch.bfloat16)
    k = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    v = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    return Case(q, k, v, causal, 1.0 / math.sqrt(D), _lens_tensor(kv_lens),
                alibi_slopes(H) if alibi else None)


# ------------------------------------------------------- fp64 and the bound

def reference_fp64(case):
    """(o, lse, A) in fp64 with the semantics of ops.reference.attention_fwd:
    ALiBi bias slope * (kv - q_pos) with q_pos = i + (len - S), len the
    slot's length under kv_lens and Skv otherwise.  A = P @ |V| is the scale
    of the error bound.  A row without a visible key gives o = 0,
    lse = -inf."""
    q, k, v = case.q.double(), case.k.double(), case.v.double()
    S, Skv = q.shape[2], k.shape[2]
    s = (q @ k.transpose(-1, -2)) * case.scale
    if case.alibi is not None:
        lens = (case.kv_lens.double() if case.kv_lens is not None
                else torch.full((B,), float(Skv), dtype=torch.float64))
        qpos = lens.view(B, 1, 1, 1) - S + \
            torch.arange(S, dtype=torch.float64).view(1, 1, S, 1)
        kpos = torch.arange(Skv, dtype=torch.float64).view(1, 1, 1, Skv)
        s = s + case.alibi.double().view(1, H, 1, 1) * (kpos - qpos)
    vis = visible(S, Skv, case.causal, case.kv_lens).expand(B, H, S, Skv)
    s = s.masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m0)
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(l > 0, l, torch.ones_like(l))
    lse = (m0 + torch.log(l)).squeeze(-1)
    return p @ v, lse, p @ v.abs()


def o_bound(A):
    """P is rounded to bf16 before the PV MFMA and o once to bf16 (unit
    roundoff 2^-8 each), everything else is fp32: per element
    |o - o_ref64| <= 2^-7 * (P @ |V|) + 1e-6."""
    return 2.0 ** -7 * A + 1e-6


def bound_ratio(o, o64, A):
    """Largest err / bound; <= 1 passes."""
    return float(((o.double() - o64).abs() / o_bound(A)).max())


# ------------------------------------------------------ tile-loop emulation

def emulate(case):
    """The kernel's loop in plain torch on the CPU: waves of 16 q rows,
    kv tiles of 64, fp32 state, the rescale taken by a whole wave when any
    of its rows has tile_max > m + 8, P rounded to bf16 for the PV product,
    V rows at or past the slot's length not loaded.

    Returns (o bf16, lse fp32, stats); stats["alphas"] holds the alpha of
    every real row in every wave that rescaled after the first tile."""
    q, k, v = case.q.float(), case.k.float(), case.v.float()
    S, Skv, D = q.shape[2], k.shape[2], q.shape[3]
    W = (S + WAVE_ROWS - 1) // WAVE_ROWS
    Sp = W * WAVE_ROWS
    qp = torch.zeros(B, H, Sp, D)
    qp[:, :, :S] = q
    real = (torch.arange(Sp) < S).view(1, 1, Sp)
    lens = (case.kv_lens.long() if case.kv_lens is not None
            else torch.full((B,), Skv, dtype=torch.long))
    qidx = torch.arange(Sp).view(1, 1, Sp, 1)
    m = torch.full((B, H, Sp), -math.inf)
    l = torch.zeros(B, H, Sp)
    acc = torch.zeros(B, H, Sp, D)
    alphas, late = [], 0
    for t in range((Skv + TILE - 1) // TILE):
        lo, hi = t * TILE, min(Skv, (t + 1) * TILE)
        kv = torch.arange(lo, hi).view(1, 1, 1, hi - lo)
        s = (qp @ k[:, :, lo:hi].transpose(-1, -2)) * case.scale
        if case.alibi is not None:
            off = (lens - S).view(B, 1, 1, 1)
            s = case.alibi.view(1, H, 1, 1) * (kv - qidx - off).float() + s
        masked = (kv >= lens.view(B, 1, 1, 1)) | (qidx >= S)
        if case.causal:
            masked = masked | (kv > qidx)
        s = s.masked_fill(masked.expand_as(s), -math.inf)
        tile_max = s.max(-1).values
        # !(tile_max <= m + THR) on any row of the wave
        trig = ~(tile_max <= m + DEFER_THR)
        trig = trig.view(B, H, W, WAVE_ROWS).any(-1, keepdim=True)
        trig = trig.expand(B, H, W, WAVE_ROWS).reshape(B, H, Sp)
        m_new = torch.maximum(m, tile_max)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m),
                            torch.exp(m - m_new))
        alpha = torch.where(trig, alpha, torch.ones_like(alpha))
        if t > 0 and bool(trig.any()):
            late += int(trig.view(B, H, W, WAVE_ROWS)[..., 0].sum())
            alphas.append(alpha[trig & real])
        m = torch.where(trig, m_new, m)
        l = l * alpha
        acc = acc * alpha.unsqueeze(-1)
        p = torch.where(torch.isinf(s), torch.zeros_like(s),
                        torch.exp(s - m.unsqueeze(-1)))
        l = l + p.sum(-1)
        vt = v[:, :, lo:hi].masked_fill(
            (kv >= lens.view(B, 1, 1, 1)).view(B, 1, hi - lo, 1), 0.0)
        acc = acc + p.to(torch.bfloat16).float() @ vt
    inv_l = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o = (acc * inv_l.unsqueeze(-1)).to(torch.bfloat16)[:, :, :S]
    lse = torch.where(l > 0, m + torch.log(l),
                      torch.full_like(l, -math.inf))[:, :, :S]
    stats = dict(late_rescales=late,
                 alphas=torch.cat(alphas) if alphas else torch.zeros(0))
    return o.contiguous(), lse.contiguous(), stats
