"""Shared by test_attention_decode_cpu.py and test_attention_decode_gpu.py:
single-query (S = 1) input builders for the split-KV decode attention kernel
with the outputs they must produce.

The exact families of attn_fwd_cases.py stop at Skv = 256 (one_hot) and at
320 visible keys (uniform), which cannot span several chunks of the decode
kernel.  The two builders here carry the same ideas to any Skv up to 65536;
the random and staircase families, the fp64 reference and the error bound
are reused from attn_fwd_cases.py with S = 1 and causal = False.

Every builder works on the CPU in bf16 and returns an attn_fwd_cases.Case;
the GPU tests move the tensors to the device."""
import math

import torch

import attn_fwd_cases as F
from attn_fwd_cases import B, H, Case

A_SCALE = F.A_SCALE   # 64
B_SCALE = F.B_SCALE

HEAD_DIMS = (16, 48, 64, 80, 96, 112, 128, 160, 256)

# (D, Skv, kv_lens) with lengths written in the kernel's chunk size C at
# that D: "1", "C-1", "C", "C+1", "2C+1", and "S" for Skv; "0" is an empty
# slot.  Every Skv of {1, C-1, C, C+1, 2C+1}, every D of HEAD_DIMS at two or
# more of them, and length pairs drawn from {0, 1, C-1, C, C+1, Skv}, among
# them an empty slot next to a full one.
EXACT_SHAPES = [
    (16, "1", None),
    (48, "1", ("0", "1")),
    (96, "1", None),
    (256, "1", None),
    (64, "C-1", None),
    (80, "C-1", ("1", "S")),
    (48, "C-1", ("C-1", "0")),
    (96, "C", None),
    (112, "C", ("C-1", "C")),
    (256, "C", ("1", "C")),
    (128, "C", ("0", "C")),
    (160, "C", None),
    (128, "C+1", None),
    (160, "C+1", ("C", "C+1")),
    (256, "C+1", ("0", "S")),
    (64, "C+1", ("C+1", "1")),
    (16, "2C+1", None),
    (48, "2C+1", ("C+1", "S")),
    (64, "2C+1", ("0", "S")),
    (80, "2C+1", ("C", "C-1")),
    (96, "2C+1", ("1", "C+1")),
    (112, "2C+1", ("S", "0")),
    (128, "2C+1", ("C-1", "C+1")),
    (160, "2C+1", None),
    (256, "2C+1", ("C", "S")),
]
# (D, alibi, kv_lens) at Skv = 2C+1
RANDOM_SHAPES = [
    (64, False, None),
    (128, True, None),
    (80, False, ("C+1", "S")),
    (128, True, ("C-1", "2C+1")),
    (256, True, ("S", "C")),
    (160, False, ("1", "C+1")),
]
STAIR_SHAPES = [(D, order) for D in (64, 128, 256)
                for order in ("asc", "desc", "shuffled")]
# (D, kv_lens) at Skv = 2C+1: a tail that starts on a chunk edge, next to an
# empty slot, and tails that start inside a chunk
TAIL_SHAPES = [
    (80, ("C", "0")),
    (128, ("C+1", "C-1")),
]
# packed-qkv and cache views: d = 80 sits inside the 128-wide instantiation,
# d = 160 inside the 256-wide one
VIEW_DIMS = (80, 160)


def length(spec, C, Skv=None):
    """The integer a length spec stands for."""
    if spec == "S":
        assert Skv is not None
        return Skv
    return {"0": 0, "1": 1, "C-1": C - 1, "C": C, "C+1": C + 1,
            "2C+1": 2 * C + 1}[spec]


def resolve(C, Skv, kv_lens):
    """(Skv, kv_lens) of a shape entry as integers."""
    n = length(Skv, C)
    if kv_lens is None:
        return n, None
    lens = tuple(length(s, C, n) for s in kv_lens)
    assert all(0 <= x <= n for x in lens)
    return n, lens


def _visible_counts(Skv, lens):
    """[B] number of visible keys per slot."""
    if lens is None:
        return torch.full((B,), Skv, dtype=torch.long)
    return lens.long()


# ------------------------------------------------------------------ one-hot

def one_hot_codes(Skv, D, gen):
    """[B, H, Skv, D] of +-1: the first ceil(log2 Skv) columns hold the bits
    of the row index, so any two rows differ somewhere; the rest is random."""
    nbits = max(1, (Skv - 1).bit_length())
    assert D >= nbits and Skv <= 65536
    code = torch.randint(0, 2, (B, H, Skv, D), generator=gen) * 2 - 1
    bits = (torch.arange(Skv).view(Skv, 1) >>
            torch.arange(nbits).view(1, nbits)) & 1
    code[..., :nbits] = (bits * 2 - 1).view(1, 1, Skv, nbits)
    return code.to(torch.bfloat16)


def one_hot(Skv, D, kv_lens=None):
    """q = k[pi] with +-1 codes and scale 64: the matched score is 64 D and
    every other visible one at least 128 lower, so in fp32 the softmax is
    exactly one-hot inside its chunk and every other chunk merges with
    weight exactly 0: o = v[pi] and lse = 64 D bit for bit."""
    gen = F._gen(11, Skv, D, *(kv_lens or ()))
    lens = F._lens_tensor(kv_lens)
    k = one_hot_codes(Skv, D, gen)
    v = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
    n_vis = _visible_counts(Skv, lens).view(B, 1).expand(B, H)
    u = torch.rand(B, H, generator=gen)
    pi = torch.minimum((u * n_vis).long(), (n_vis - 1).clamp(min=0))
    empty = n_vis == 0
    idx = pi.view(B, H, 1, 1).expand(B, H, 1, D)
    q = k.gather(2, idx)
    o = v.gather(2, idx).clone()
    o[empty] = 0
    lse = torch.full((B, H, 1), A_SCALE * D, dtype=torch.float32)
    lse[empty] = -math.inf

    # builder's own check: the gap, in fp64, on every visible pair
    s = (q.double() @ k.double().transpose(-1, -2)) * A_SCALE   # [B,H,1,Skv]
    vis = F.visible(1, Skv, False, lens).expand(B, H, 1, Skv)
    matched = torch.zeros(B, H, 1, Skv, dtype=torch.bool)
    matched.scatter_(3, pi.view(B, H, 1, 1), True)
    live = ~empty
    assert bool((s[matched].view(B, H)[live] == A_SCALE * D).all())
    others = s.masked_fill(matched | ~vis, -math.inf)
    gap = (A_SCALE * D - others.max(-1).values).view(B, H)
    assert bool((gap[live] >= 128.0).all()), "one-hot gap below 128"
    return Case(q, k, v, False, A_SCALE, lens, None, o, lse,
                dict(pi=pi, min_gap=float(gap[live].min())
                     if bool(live.any()) else math.inf))


# ------------------------------------------------------------------ uniform

def _uniform_ok(sums, n, o):
    """Both ways a kernel may normalise, in fp32, round to the expected
    bf16: sum * (1 / n) and sum / n."""
    s32 = sums.to(torch.float32)
    n32 = n.to(torch.float32).clamp(min=1)
    by_mul = (s32 * (1.0 / n32)).to(torch.bfloat16)
    by_div = (s32 / n32).to(torch.bfloat16)
    return bool(torch.equal(by_mul, o)) and bool(torch.equal(by_div, o))


def uniform(Skv, D, kv_lens=None):
    """q = 0: every visible key weighs 1/n, so o = bf16(sum of the visible
    ternary v / n) with an exact integer sum, and lse = log n.  The values
    are drawn again (salt 0, 1, ..) until the expected bf16 does not depend
    on how the kernel normalises; the salt taken is in info."""
    lens = F._lens_tensor(kv_lens)
    n = _visible_counts(Skv, lens).view(B, 1, 1).expand(B, H, 1)
    vis = F.visible(1, Skv, False, lens).expand(B, H, 1, Skv)
    for salt in range(16):
        gen = F._gen(12, Skv, D, salt, *(kv_lens or ()))
        k = torch.randn(B, H, Skv, D, generator=gen).to(torch.bfloat16)
        v = F.ternary(gen, B, H, Skv, D)
        sums = vis.double() @ v.double()                       # [B, H, 1, D]
        assert bool((sums == sums.round()).all())
        assert float(sums.abs().max()) < 2 ** 24
        nd = n.unsqueeze(-1).double()
        o = torch.where(nd > 0, sums / nd.clamp(min=1),
                        torch.zeros_like(sums)).to(torch.bfloat16)
        if _uniform_ok(sums, n.unsqueeze(-1), o):
            break
    else:
        raise AssertionError("no salt gives a normalisation-free expectation")
    q = torch.zeros(B, H, 1, D, dtype=torch.bfloat16)
    lse64 = torch.log(n.double())                               # log 0 = -inf
    return Case(q, k, v, False, B_SCALE, lens, None, o,
                lse64.to(torch.float32), dict(n=n, lse64=lse64, salt=salt))


# ------------------------------------------------------- random, staircase

def random_case(Skv, D, alibi, kv_lens=None):
    return F.random_case(1, Skv, D, False, alibi, kv_lens)


def staircase(Skv, D, order):
    """The single query row has g = 9: a step of 9 in the scores every 64
    keys, so chunks merge with weights far from 1 in every order."""
    return F.staircase(1, Skv, D, False, order)


def o_bound(A):
    """The project's bound for attention outputs (attn_fwd_cases.o_bound).
    The decode kernel does not round P, so it should sit well inside."""
    return F.o_bound(A)
