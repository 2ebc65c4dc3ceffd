"""The e4m3 KV cache on the GPU: the quantize-and-append kernel
(csrc/kv_cache_fp8.hip) on rows with exactly known bytes and on random rows,
the e4m3 split-KV decode kernel (csrc/attention_decode_fp8.hip) against fp64
over the dequantized cache, its blindness past kv_lens, its bit invariance,
strided views, graph capture, and the decoders with the cache turned on.
B = H = 2 throughout; lengths are written in C = ops.DECODE_ATTN_CHUNK(D).
Measured err/bound ratios: docs/KERNELS.md, "e4m3 KV cache"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_decode_cases as DC
import attn_fwd_cases as F
import kv_fp8_cases as KC
from alpa_amd import ops
from alpa_amd.global_env import global_config
from alpa_amd.ops import reference as ref

B, H = F.B, F.H
NAN_BYTE = 0x7F


def _packed_kv(k, v):
    """k, v [B, H, S, d] as views of a packed [B, S, H, 3, d] projection on
    the GPU whose other entries are NaN."""
    Bk, Hk, S, d = k.shape
    qkv = torch.full((Bk, S, Hk, 3, d), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    qkv[:, :, :, 1] = k.cuda().permute(0, 2, 1, 3)
    qkv[:, :, :, 2] = v.cuda().permute(0, 2, 1, 3)
    return qkv[:, :, :, 1].permute(0, 2, 1, 3), \
        qkv[:, :, :, 2].permute(0, 2, 1, 3)


def _nan_cache(L, d, extra=0):
    """(k8, k_scale, v8, v_scale) of capacity L, all NaN, as views of
    buffers `extra` rows longer."""
    def half():
        c8 = torch.full((B, H, L + extra, d), NAN_BYTE, dtype=torch.uint8,
                        device="cuda").view(torch.float8_e4m3fn)
        cs = torch.full((B, H, L + extra), float("nan"), device="cuda")
        return c8[:, :, :L], cs[:, :, :L]
    return half() + half()


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}
                  [t.element_size()])


def _cat(a, b):
    """Along the cache axis; bytes are joined as uint8."""
    if a.element_size() > 1:
        return torch.cat([a, b], 2)
    return torch.cat([_bits(a), _bits(b)], 2).view(torch.float8_e4m3fn)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("pos", ["int", "tensor"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", [16, 80, 128, 256])
def test_append_exact(d, S, pos):
    """Rows of e4m3-representable values times 2^j with one +-448 * 2^j
    entry: every division is exact, so the bytes are the codes and the scale
    is 2^j, bit for bit."""
    gen = torch.Generator().manual_seed(d * 10 + S)
    codes = torch.randint(0, 256, (2, B, H, S, d), generator=gen,
                          dtype=torch.uint8)
    codes[((codes & 0x7F) == NAN_BYTE) | (codes == 0x80)] = 0   # NaN, -0
    peak = torch.randint(0, d, (2, B, H, S, 1), generator=gen)
    sign = torch.randint(0, 2, (2, B, H, S, 1), generator=gen) * 0x80
    codes.scatter_(-1, peak, (0x7E + sign).to(torch.uint8))
    two_j = torch.exp2(torch.randint(-8, 9, (2, B, H, S), generator=gen)
                       .float())
    x = (codes.view(torch.float8_e4m3fn).float() *
         two_j.unsqueeze(-1)).bfloat16()
    k, v = _packed_kv(x[0], x[1])
    L = 8
    at = [2, 2] if pos == "int" else [1, 4]
    k8, ks, v8, vs = cache = _nan_cache(L, d)
    ops.kv_cache_append_fp8(k, v, *cache, 2 if pos == "int" else
                            torch.tensor(at, device="cuda"))
    for i, (c8, cs) in enumerate(((k8, ks), (v8, vs))):
        for b in range(B):
            rows = slice(at[b], at[b] + S)
            assert torch.equal(c8[b, :, rows].view(torch.uint8).cpu(),
                               codes[i, b])
            assert torch.equal(cs[b, :, rows].cpu(), two_j[i, b])


def test_append_random():
    """Random rows of many magnitudes and one zero row, into slot 0 at rows
    1..3; slot 1 sits at pos = max_len and writes nothing.  Every other row,
    and the buffer past max_len, keeps its NaN prefill bit for bit."""
    d, S, L = 80, 3, 6
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(2, B, H, S, d, generator=gen) * torch.exp2(
        torch.randint(-12, 12, (2, B, H, S, 1), generator=gen).float())
    ).bfloat16()
    x[0, 0, 1, 2] = 0
    k, v = _packed_kv(x[0], x[1])
    cache = _nan_cache(L, d, extra=2)
    before = [t._base.clone() for t in cache]
    ops.kv_cache_append_fp8(k, v, *cache,
                            torch.tensor([1, L], device="cuda",
                                         dtype=torch.int32))
    for i in range(2):
        c8, cs = cache[2 * i], cache[2 * i + 1]
        KC.check_rows(x[i, 0], c8[0, :, 1:4], cs[0, :, 1:4])
        q, sc = ref.kv_quantize_rows(x[i, 0])
        assert _same((c8[0, :, 1:4].cpu(), cs[0, :, 1:4].cpu()), (q, sc))
    for t, old in zip(cache, before):
        now = t._base.clone()
        now[0, :, 1:4] = old[0, :, 1:4]
        assert _same([now], [old])


def _quantized(D, kv_lens, alibi=False, Skv="2C+1"):
    """A random decode case whose k, v are the dequantized e4m3 rows, so the
    quantization error is on neither side of a comparison, with its cache
    (k8, k_scale, v8, v_scale) on the GPU."""
    n, lens = DC.resolve(ops.DECODE_ATTN_CHUNK(D), Skv, kv_lens)
    case = DC.random_case(n, D, alibi, lens)
    halves = ref.kv_quantize_rows(case.k) + ref.kv_quantize_rows(case.v)
    case.k = ref.kv_dequantize_rows(*halves[:2])
    case.v = ref.kv_dequantize_rows(*halves[2:])
    return case, tuple(t.cuda() for t in halves)


def _run(case, cache, kv_lens="case", q=None):
    from alpa_amd.ops._backend import hip_ops
    lens = case.kv_lens if isinstance(kv_lens, str) else kv_lens
    q = case.q.cuda() if q is None else q
    assert ops.decode_attn_fp8_ok(q, *cache)
    o, lse = hip_ops().attn_decode_fp8(
        q, *cache, case.scale,
        None if case.alibi is None else case.alibi.cuda(),
        None if lens is None else lens.cuda())
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("kv_lens", [("C-1", "2C+1"), ("C+1", "0"), None])
@pytest.mark.parametrize("D", [64, 80, 128, 256])
def test_decode_against_fp64(D, kv_lens):
    case, cache = _quantized(D, kv_lens, alibi=D == 80)
    o, lse = _run(case, cache)
    o64, lse64, A = F.reference_fp64(case)
    ratio = F.bound_ratio(o, o64, A)
    live = torch.isfinite(lse64)
    lse_err = float((lse.double() - lse64)[live].abs().max())
    print(f"fp8 decode D={D} lens={kv_lens}: err/bound {ratio:.3f}, "
          f"lse err {lse_err:.2g}")
    assert ratio <= 1.0 and lse_err <= F.LSE_ATOL
    assert bool((lse[~live] == -float("inf")).all())
    assert bool((o[~live.squeeze(-1)] == 0).all())


def _poison_tail(cache, lens, byte, scale):
    """A copy with `byte` / `scale` at and past each slot's length."""
    out = [t.clone() for t in cache]
    for b in range(B):
        for c8, cs in (out[:2], out[2:]):
            c8.view(torch.uint8)[b, :, lens[b]:] = byte
            cs[b, :, lens[b]:] = scale
    return out


def test_decode_ignores_the_tail():
    case, cache = _quantized(128, ("C+1", "C-1"), alibi=True)
    lens = case.kv_lens.tolist()
    assert _same(_run(case, _poison_tail(cache, lens, NAN_BYTE, float("nan"))),
                 _run(case, _poison_tail(cache, lens, 0, 0.0)))


def test_decode_invariance():
    """Each slot alone and sliced to its length, the cache padded by three
    chunks of NaN, and a length-10 slot in one chunk against four."""
    D = 80
    C = ops.DECODE_ATTN_CHUNK(D)
    case, cache = _quantized(D, ("C-1", "2C+1"))
    o, lse = _run(case, cache)
    for b, n in enumerate(case.kv_lens.tolist()):
        alone = _run(case, [t[b:b + 1, :, :n] for t in cache], None,
                     case.q[b:b + 1].cuda())
        assert _same(alone, (o[b:b + 1], lse[b:b + 1]))
    pad = _nan_cache(3 * C, D)
    assert _same(_run(case, [_cat(t, p) for t, p in zip(cache, pad)]),
                 (o, lse))
    case4, cache4 = _quantized(D, None, Skv="2C+1")
    ten = torch.full((B,), 10, dtype=torch.int32)
    wide = [_cat(t, p) for t, p in zip(cache4, pad)]
    assert _same(_run(case4, [t[:, :, :C].contiguous() for t in cache4], ten),
                 _run(case4, [t[:, :, :4 * C] for t in wide], ten))


def test_decode_strided_views():
    D = 160
    case, cache = _quantized(D, ("C+1", "2C+1"))
    qkv = torch.randn(B, 1, H, 3, D, device="cuda").bfloat16()
    q = qkv[:, :, :, 0].permute(0, 2, 1, 3)
    assert not q.is_contiguous()
    total = cache[0].shape[2]
    big = [_cat(t, t)[:, :, :total] for t in cache]
    assert not big[0].is_contiguous()
    assert _same(_run(case, big, q=q), _run(case, cache, q=q.contiguous()))


def test_capture_append_and_decode():
    """Append plus decode captured once with device pos and kv_lens; every
    replay after add_(1) equals the eager result for the new lengths."""
    D, L, n0 = 128, 140, 126          # the replays cross the chunk edge
    gen = torch.Generator().manual_seed(5)
    hist = torch.randn(2, B, H, n0, D, generator=gen).bfloat16().cuda()
    steps = torch.randn(4, 3, B, H, 1, D, generator=gen).bfloat16().cuda()
    q, k, v = (steps[0, i].clone() for i in range(3))
    pos = torch.tensor([n0, n0 - 5], device="cuda")
    lens = (pos + 1).int()
    graph_c, eager_c = _nan_cache(L, D), _nan_cache(L, D)
    for c in (graph_c, eager_c):
        ops.kv_cache_append_fp8(hist[0], hist[1], *c, 0)

    def step(cache):
        ops.kv_cache_append_fp8(k, v, *cache, pos)
        return ops.flash_attention_decode_fp8(q, *cache, kv_lens=lens)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(graph_c)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_graph = step(graph_c)
    for i in range(4):
        for dst, src in zip((q, k, v), steps[i]):
            dst.copy_(src)
        if i:
            pos.add_(1)
            lens.add_(1)
        graph.replay()
        assert _same([o_graph], [step(eager_c)])
        assert bool(torch.isfinite(o_graph.float()).all())


@pytest.mark.parametrize("name", ["codegen", "bloom"])
def test_model_with_fp8_cache(monkeypatch, name):
    """Prefill, then one cached step, against the full forward of the same
    bf16 model.  Tolerance: the 5e-2 (rtol and atol) this comparison has in
    bf16 with a bf16 cache, plus twice the effect of the e4m3 cache alone as
    measured on the fp32 CPU model (kv_fp8_cases.EFFECT: 0.0543 CodeGen,
    0.0549 BLOOM), so atol 0.159 / 0.160.  And the captured decode loop
    returns the tokens of the eager one (BLOOM: CodeGen's rotary has no
    per-slot positions, so it has no captured loop with any cache)."""
    monkeypatch.setattr(global_config, "kv_cache_fp8", True)
    m = KC.tiny_model(name, torch.bfloat16, "cuda")
    inc, full = KC.cached_step_and_full(m, name)
    print(f"{name}: max |cached - full| {float((inc - full).abs().max()):.4f}")
    torch.testing.assert_close(inc, full, rtol=5e-2,
                               atol=5e-2 + 2 * KC.EFFECT[name])
    if name != "bloom":
        return
    ids = torch.randint(0, KC.VOCAB[name], (2, 9), device="cuda")
    assert torch.equal(m.generate_graphed(ids, 6),
                       m.generate(ids, max_new_tokens=6))
