"""The split-KV MFMA chunk attention kernel (csrc/attention_chunk.hip) on the
GPU, over the bf16 and the e4m3 cache: random inputs against fp64 within the
project's bound, exact key counts, blindness past kv_lens, bit invariance,
strided views, the public op in pieces and under graph capture, and a
decoder prefilled in two chunks.  B = H = 2 throughout; lengths are written
in C = ops.DECODE_ATTN_CHUNK(D) and Sq."""
import math
from types import SimpleNamespace

import pytest
import torch

import attn_fwd_cases as F
from alpa_amd import ops
from alpa_amd.models.bloom import alibi_slopes
from alpa_amd.ops import reference as ref
from alpa_amd.ops._backend import hip_ops

pytestmark = pytest.mark.gpu
B, H = F.B, F.H
FP8 = torch.float8_e4m3fn

# slot lengths as a*C + b + c*Sq: the causal edge across a chunk boundary
# (rows that see no key of the last chunk), on one, no history, leading rows
# empty, nothing at all
LENS = {"edge": (1, 3, 0), "C": (1, 0, 0), "2C": (2, 0, 0), "Sq": (0, 0, 1),
        "short": (0, -1, 1), "zero": (0, 0, 0)}
PAIRS = [("edge", "zero"), ("C", "short"), ("2C", "Sq")]
# (cache, D, Sq, alibi, length of slot 0, of slot 1)
RANDOM = [
    ("bf16", 64, 1, False, "edge", "zero"),
    ("bf16", 80, 15, True, "C", "short"),
    ("bf16", 128, 17, False, "2C", "Sq"),
    ("bf16", 256, 64, True, "edge", "2C"),
    ("bf16", 128, 33, True, "edge", "short"),
    ("bf16", 64, 16, False, "C", "edge"),
    ("bf16", 256, 2, False, "Sq", "2C"),
    ("e4m3", 64, 2, True, "edge", "Sq"),
    ("e4m3", 80, 16, False, "2C", "zero"),
    ("e4m3", 128, 64, True, "C", "edge"),
    ("e4m3", 256, 33, False, "edge", "short"),
    ("e4m3", 256, 17, True, "2C", "C"),
    ("e4m3", 128, 1, False, "short", "edge"),
    ("e4m3", 64, 15, False, "Sq", "2C"),
]


def make(cache, D, Sq, names, alibi=False, Skv=None, zero_q=False):
    """Operands on the GPU, the cache as the list the extension takes
    ([k, v] or [k8, k_scale, v8, v_scale]), and k, v in fp64 as the cache
    holds them."""
    C = ops.DECODE_ATTN_CHUNK(D)
    Skv = Skv or 2 * C + 1
    g = torch.Generator().manual_seed(1000 * D + 10 * Sq + len(cache))
    q, k, v = (torch.randn(B, H, n, D, generator=g).to(torch.bfloat16)
               for n in (Sq, Skv, Skv))
    if zero_q:
        q.zero_()
    lens = torch.tensor([min(a * C + b + c * Sq, Skv)
                         for a, b, c in (LENS[n] for n in names)],
                        dtype=torch.int32)
    if cache == "e4m3":
        (k8, ks), (v8, vs) = ref.kv_quantize_rows(k), ref.kv_quantize_rows(v)
        kv = [k8, ks, v8, vs]
        k, v = ref.kv_dequantize_rows(k8, ks), ref.kv_dequantize_rows(v8, vs)
    else:
        kv = [k, v]
    return SimpleNamespace(q=q.cuda(), kv=[t.cuda() for t in kv], lens=lens,
                           k64=k.double(), v64=v.double(), scale=D ** -0.5,
                           slopes=alibi_slopes(H) if alibi else None)


def run(c, q=None, kv=None, lens="own"):
    kv = c.kv if kv is None else kv
    fn = hip_ops().attn_chunk if len(kv) == 2 else hip_ops().attn_chunk_fp8
    lens = c.lens if isinstance(lens, str) else lens
    return fn(c.q if q is None else q, *kv, c.scale,
              None if c.slopes is None else c.slopes.cuda(),
              None if lens is None else lens.cuda())


def ref64(c, q=None):
    """(o, lse, P @ |V|) in fp64 under the bottom-right causal mask."""
    q = (c.q if q is None else q).cpu().double()
    Sq, Skv = q.shape[2], c.k64.shape[2]
    pos = c.lens.long().view(B, 1, 1, 1) - Sq + \
        torch.arange(Sq).view(1, 1, Sq, 1)
    kv = torch.arange(Skv).view(1, 1, 1, Skv)
    s = (q @ c.k64.transpose(-1, -2)) * c.scale
    if c.slopes is not None:
        s = s + c.slopes.double().view(1, H, 1, 1) * (kv - pos)
    s = s.masked_fill(kv > pos, -math.inf)
    m = s.max(-1, keepdim=True).values
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m0)
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(l > 0, l, torch.ones_like(l))
    return p @ c.v64, (m0 + torch.log(l)).squeeze(-1), p @ c.v64.abs()


def check_against_fp64(c, o, lse, tag, q=None):
    o64, lse64, A = ref64(c, q)
    o, lse = o.cpu(), lse.cpu().double()
    ratio = F.bound_ratio(o, o64, A)
    empty = torch.isinf(lse64)
    lse_err = float((lse - lse64)[~empty].abs().max()) if (~empty).any() else 0
    print(f"{tag}: err/bound {ratio:.3f}, lse err {lse_err:.2e}")
    assert ratio <= 1.0
    assert lse_err <= F.LSE_ATOL
    assert bool((lse[empty] == -math.inf).all())
    assert bool((o[empty] == 0).all())


def same_bits(a, b):
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def poison_(t):
    """NaN everywhere, in place (e4m3: the NaN code 0x7F)."""
    if t.dtype == FP8:
        t.view(torch.uint8).fill_(0x7F)
    else:
        t.fill_(math.nan)


def widened(t, n):
    """t with its key axis (dim 2) widened to n rows of NaN: a view of the
    first rows of a larger cache."""
    shape = list(t.shape)
    shape[2] = n
    big = torch.empty(shape, dtype=torch.uint8 if t.dtype == FP8 else t.dtype,
                      device=t.device)
    big = big.view(FP8) if t.dtype == FP8 else big
    poison_(big)
    big[:, :, :t.shape[2]] = t
    return big


@pytest.mark.parametrize("cache,D,Sq,alibi,la,lb", RANDOM)
def test_random_against_fp64(cache, D, Sq, alibi, la, lb):
    c = make(cache, D, Sq, (la, lb), alibi)
    o, lse = run(c)
    check_against_fp64(c, o, lse, f"{cache} D{D} Sq{Sq} {la}/{lb}")


@pytest.mark.parametrize("cache,D,Sq", [("bf16", 64, 17), ("e4m3", 128, 33),
                                        ("bf16", 256, 64), ("e4m3", 80, 1),
                                        ("bf16", 128, 16)])
def test_counts_exactly(cache, D, Sq):
    """q = 0: every visible key weighs the same, lse = log(count)."""
    for names in PAIRS:
        c = make(cache, D, Sq, names, zero_q=True)
        lse = run(c)[1].cpu()
        n = (c.lens.long().view(B, 1, 1) - Sq + 1 +
             torch.arange(Sq).view(1, 1, Sq)).clamp(min=0).expand(B, H, Sq)
        want = torch.log(n.double())
        live = n > 0
        assert bool((lse[~live] == -math.inf).all()), names
        assert float((lse.double() - want)[live].abs().max()) <= 1e-4, names


@pytest.mark.parametrize("cache,D,Sq,la,lb", [
    ("bf16", 128, 17, "edge", "Sq"), ("e4m3", 64, 33, "C", "short"),
    ("e4m3", 256, 2, "edge", "zero"), ("bf16", 80, 64, "2C", "edge")])
def test_tail_is_ignored_and_bits_are_invariant(cache, D, Sq, la, lb):
    c = make(cache, D, Sq, (la, lb), alibi=True)
    base = run(c)
    assert same_bits(run(c), base)                       # run to run
    # NaN in k, v and the scales at and past each slot's length
    kv = [t.clone() for t in c.kv]
    for b in range(B):
        for t in kv:
            poison_(t[b, :, int(c.lens[b]):])
    assert same_bits(run(c, kv=kv), base)
    # the cache as a view of one with 3 more chunks of NaN
    C = ops.DECODE_ATTN_CHUNK(D)
    Skv = c.kv[0].shape[2]
    assert same_bits(run(c, kv=[widened(t, Skv + 3 * C) for t in c.kv]), base)
    # each slot alone, cut to its length, without kv_lens
    for b in range(B):
        n = int(c.lens[b])
        o, lse = run(c, q=c.q[b:b + 1],
                     kv=[t[b:b + 1, :, :n].contiguous() for t in c.kv],
                     lens=None)
        assert same_bits((o, lse), (base[0][b:b + 1], base[1][b:b + 1])), b


@pytest.mark.parametrize("cache,D", [("bf16", 64), ("e4m3", 256),
                                     ("bf16", 256), ("e4m3", 64)])
def test_strided_operands(cache, D):
    """q out of a packed [B, Sq, H, 3, d] projection, the cache as the first
    rows of a larger one."""
    Sq = 17
    c = make(cache, D, Sq, ("edge", "2C"))
    qkv = torch.zeros(B, Sq, H, 3, D, dtype=torch.bfloat16, device="cuda")
    qkv[:, :, :, 0] = c.q.permute(0, 2, 1, 3)
    q = qkv[:, :, :, 0].permute(0, 2, 1, 3)
    Skv = c.kv[0].shape[2]
    kv = [widened(t, Skv + 7)[:, :, :Skv] for t in c.kv]
    assert not q.is_contiguous() and not kv[0].is_contiguous()
    assert same_bits(run(c, q=q, kv=kv), run(c))


@pytest.mark.parametrize("cache,D,Sq", [("bf16", 128, 65), ("e4m3", 64, 130),
                                        ("bf16", 80, 130), ("e4m3", 256, 65)])
def test_public_op_in_pieces(cache, D, Sq):
    """Sq = 65 and 130 run as two and three launches, with and without
    lengths."""
    C = ops.DECODE_ATTN_CHUNK(D)
    c = make(cache, D, Sq, ("edge", "2C"), alibi=True, Skv=2 * C + 1)
    op = ops.flash_attention_chunk if cache == "bf16" \
        else ops.flash_attention_chunk_fp8
    assert (ops.chunk_attn_ok if cache == "bf16"
            else ops.chunk_attn_fp8_ok)(c.q, *c.kv)
    sl = c.slopes.cuda()
    o = op(c.q, *c.kv, kv_lens=c.lens.cuda(), scale=c.scale, alibi_slopes=sl)
    o64, _, A = ref64(c)
    ratio = F.bound_ratio(o.cpu(), o64, A)
    c.lens = torch.full((B,), 2 * C + 1, dtype=torch.int32)
    o = op(c.q, *c.kv, scale=c.scale, alibi_slopes=sl)
    o64, _, A = ref64(c)
    ratio2 = F.bound_ratio(o.cpu(), o64, A)
    print(f"{cache} D{D} Sq{Sq}: err/bound {ratio:.3f}, {ratio2:.3f}")
    assert ratio <= 1.0 and ratio2 <= 1.0


@pytest.mark.parametrize("cache", ["bf16", "e4m3"])
def test_graph_capture_with_device_lengths(cache):
    D, Sq = 128, 70
    C = ops.DECODE_ATTN_CHUNK(D)
    c = make(cache, D, Sq, ("edge", "C"))
    op = ops.flash_attention_chunk if cache == "bf16" \
        else ops.flash_attention_chunk_fp8
    lens = c.lens.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op(c.q, *c.kv, kv_lens=lens, scale=c.scale)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(c.q, *c.kv, kv_lens=lens, scale=c.scale)
    for _ in range(3):
        graph.replay()
        eager = op(c.q, *c.kv, kv_lens=lens, scale=c.scale)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
        lens.add_(1)
    assert int(lens[0]) == C + 6


def test_opt_prefill_in_two_chunks():
    """A bf16 OPT prefilled as 9 + 7 tokens against one pass of 16: the same
    greedy token, logits within the bf16 model tolerance of
    test_kernels_gpu.py (rtol = atol = 5e-2)."""
    import alpa_amd as aa
    from alpa_amd.models.opt import OPTConfig, OPTModel
    aa.init()
    cfg = OPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                    vocab_size=512, max_seq_len=128)
    m = OPTModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=4)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 512, (2, 16), generator=g).cuda()
    with torch.no_grad():
        whole = m.forward_step(ids, m.new_cache(2))
        cache = m.new_cache(2)
        m.forward_step(ids[:, :9], cache)
        parts = m.forward_step(ids[:, 9:], cache)
    print(f"max |chunked - whole| "
          f"{float((parts.float() - whole.float()).abs().max()):.3e} of "
          f"max |logit| {float(whole.float().abs().max()):.3f}")
    assert torch.equal(m.greedy_token(parts), m.greedy_token(whole))
    torch.testing.assert_close(parts.float(), whole.float(), rtol=5e-2,
                               atol=5e-2)
