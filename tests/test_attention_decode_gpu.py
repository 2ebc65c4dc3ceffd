"""The split-KV decode attention kernel (csrc/attention_decode.hip) on inputs
with exactly known outputs around its chunk edges, against fp64, with
poisoned memory past kv_lens, through strided views, under graph capture,
and its bit invariance: a slot's o and lse depend on that slot alone.

Families (attn_decode_cases.py), all at S = 1, B = H = 2, with lengths
written in C = ops.DECODE_ATTN_CHUNK(D):

  one-hot    o = v[pi] and lse = 64 D bit for bit over any number of chunks:
             key and value indexing, head-dim columns, the merge with
             weights exactly 0 and 1
  uniform    o = bf16(sum of visible v / n) bit for bit, lse = log n: masks,
             counts, the merge with every weight 1
  staircase  chunks that merge with weights far from 1, against fp64
  random     ALiBi and kv_lens combinations, against fp64

Measured err/bound on MI355X with the project's bound
2^-7 * (P @ |V|) + 1e-6: see docs/KERNELS.md."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_decode_cases as DC
import attn_fwd_cases as F
from alpa_amd import ops

B, H = F.B, F.H


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _dev(t):
    return None if t is None else t.cuda()


def _shape(D, Skv, kv_lens):
    return DC.resolve(ops.DECODE_ATTN_CHUNK(D), Skv, kv_lens)


def _run(ext, case, kv_lens="case"):
    """(o, lse) of the kernel, back on the CPU."""
    lens = case.kv_lens if isinstance(kv_lens, str) else kv_lens
    o, lse = ext.attn_decode(_dev(case.q), _dev(case.k), _dev(case.v),
                             case.scale, _dev(case.alibi), _dev(lens))
    assert o.shape == case.q.shape and o.dtype == torch.bfloat16
    assert lse.shape == case.q.shape[:3] and lse.dtype == torch.float32
    return o.cpu(), lse.cpu()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _check_uniform(o, lse, case):
    assert torch.equal(o, case.o)
    n = case.info["n"]
    some = n > 0
    assert bool((lse[~some] == -math.inf).all())
    err = (lse.double() - case.info["lse64"])[some].abs()
    worst = float(err.max()) if err.numel() else 0.0
    print(f"uniform lse err {worst:.3g}")
    assert worst <= 1e-4


def _check_fp64(o, lse, case):
    o64, lse64, A = F.reference_fp64(case)
    ratio = F.bound_ratio(o, o64, A)
    lse_err = float((lse.double() - lse64).abs().max())
    print(f"err/bound {ratio:.3f}  lse err {lse_err:.3g}")
    assert ratio <= 1.0
    torch.testing.assert_close(lse.double(), lse64, rtol=0, atol=F.LSE_ATOL)


def test_chunk_constant_matches_the_kernel(ext):
    for D in DC.HEAD_DIMS:
        assert ext.attn_decode_chunk(D) == ops.DECODE_ATTN_CHUNK(D)


@pytest.mark.parametrize("D,Skv,kv_lens", DC.EXACT_SHAPES)
def test_one_hot(ext, D, Skv, kv_lens):
    """An empty slot gives o = 0 and lse = -inf."""
    n, lens = _shape(D, Skv, kv_lens)
    case = DC.one_hot(n, D, lens)
    o, lse = _run(ext, case)
    assert torch.equal(lse, case.lse)
    assert torch.equal(o, case.o)


@pytest.mark.parametrize("D,Skv,kv_lens", DC.EXACT_SHAPES)
def test_uniform(ext, D, Skv, kv_lens):
    n, lens = _shape(D, Skv, kv_lens)
    case = DC.uniform(n, D, lens)
    _check_uniform(*_run(ext, case), case)


@pytest.mark.parametrize("D,alibi,kv_lens", DC.RANDOM_SHAPES)
def test_random(ext, D, alibi, kv_lens):
    n, lens = _shape(D, "2C+1", kv_lens)
    case = DC.random_case(n, D, alibi, lens)
    _check_fp64(*_run(ext, case), case)


@pytest.mark.parametrize("D,order", DC.STAIR_SHAPES)
def test_staircase(ext, D, order):
    n, _ = _shape(D, "2C+1", None)
    case = DC.staircase(n, D, order)
    _check_fp64(*_run(ext, case), case)


@pytest.mark.parametrize("value", [math.nan, math.inf])
@pytest.mark.parametrize("which", ["v", "k"])
@pytest.mark.parametrize("D,kv_lens", DC.TAIL_SHAPES)
def test_tail_is_ignored(ext, D, kv_lens, which, value):
    """Memory at and past kv_lens[b] is never observed: NaN or Inf there
    gives the same bits as zeros."""
    n, lens = _shape(D, "2C+1", kv_lens)
    case = DC.uniform(n, D, lens)
    clean = _run(ext, F.poison_tail(case, which, 0.0))
    dirty = _run(ext, F.poison_tail(case, which, value))
    assert _same_bits(dirty, clean)
    _check_uniform(*dirty, case)


# ------------------------------------------------------------- invariance

INVARIANCE_SHAPES = [
    (128, True, ("C-1", "2C+1")),
    (80, False, ("C+1", "S")),
    (256, True, ("C", "0")),
    (64, False, None),
]


@pytest.fixture(scope="module", params=INVARIANCE_SHAPES,
                ids=lambda p: f"D{p[0]}-alibi{int(p[1])}-{p[2]}")
def inv(ext, request):
    """(case, its lengths as a list, the kernel's (o, lse) for it)."""
    D, alibi, kv_lens = request.param
    n, lens = _shape(D, "2C+1", kv_lens)
    case = DC.random_case(n, D, alibi, lens)
    return case, list(lens or (n, n)), _run(ext, case)


def test_invariant_to_cache_capacity(ext, inv):
    """(a) k and v padded with 3 chunks of NaN: same bits."""
    case, lens, want = inv
    C = ops.DECODE_ATTN_CHUNK(case.q.shape[3])
    pad = torch.full((B, H, 3 * C, case.q.shape[3]), math.nan,
                     dtype=torch.bfloat16)
    wide = F.Case(case.q, torch.cat([case.k, pad], 2),
                  torch.cat([case.v, pad], 2), False, case.scale,
                  torch.tensor(lens, dtype=torch.int32), case.alibi)
    assert _same_bits(_run(ext, wide), want)


def test_invariant_to_the_other_slots(ext, inv):
    """(b) each slot alone, k and v sliced to its length, no kv_lens."""
    case, lens, (o, lse) = inv
    for b, L in enumerate(lens):
        alone = F.Case(case.q[b:b + 1], case.k[b:b + 1, :, :L],
                       case.v[b:b + 1, :, :L], False, case.scale, None,
                       case.alibi)
        ob, lseb = ext.attn_decode(alone.q.cuda(), alone.k.cuda(),
                                   alone.v.cuda(), alone.scale,
                                   _dev(alone.alibi), None)
        assert _same_bits((ob.cpu(), lseb.cpu()), (o[b:b + 1], lse[b:b + 1]))


def test_full_lengths_equal_no_lengths(ext):
    """(c) kv_lens = [Skv, Skv] against kv_lens = None."""
    n, _ = _shape(128, "2C+1", None)
    case = DC.random_case(n, 128, True, None)
    full = torch.full((B,), n, dtype=torch.int32)
    assert _same_bits(_run(ext, case, full), _run(ext, case, None))


def test_two_calls_agree(ext, inv):
    """(d) two successive calls."""
    case, _, want = inv
    assert _same_bits(_run(ext, case), want)


def test_short_slot_in_a_long_cache(ext):
    """A slot of length 10 gives the same bits in a cache of 10 keys (one
    chunk, finished by the partial kernel itself) and of 4 C keys (two
    launches)."""
    D = 64
    C = ops.DECODE_ATTN_CHUNK(D)
    case = DC.random_case(4 * C, D, False, (10, C))
    o, lse = _run(ext, case)
    short = F.Case(case.q[:1], case.k[:1, :, :10].contiguous(),
                   case.v[:1, :, :10].contiguous(), False, case.scale)
    o1, lse1 = ext.attn_decode(short.q.cuda(), short.k.cuda(),
                               short.v.cuda(), short.scale, None, None)
    assert _same_bits((o1.cpu(), lse1.cpu()), (o[:1], lse[:1]))


# ---------------------------------------------------------------- strides

@pytest.mark.parametrize("d", DC.VIEW_DIMS)
def test_strided_operands(ext, d):
    """k and v as [:, :, :total] views of a larger cache and q as the view
    of a packed [B, 1, H, 3, d] projection, read in place: the bits of the
    contiguous call."""
    C = ops.DECODE_ATTN_CHUNK(d)
    total = C + 3
    case = DC.random_case(total, d, False, (total, C - 1))
    want = _run(ext, case)
    cache_k = torch.full((B, H, total + 37, d), math.nan,
                         dtype=torch.bfloat16, device="cuda")
    cache_v = torch.full_like(cache_k, math.nan)
    cache_k[:, :, :total] = case.k.cuda()
    cache_v[:, :, :total] = case.v.cuda()
    qkv = torch.full((B, 1, H, 3, d), math.nan, dtype=torch.bfloat16,
                     device="cuda")
    qkv[:, :, :, 0] = case.q.permute(0, 2, 1, 3).cuda()
    q = qkv[:, :, :, 0].permute(0, 2, 1, 3)
    kc, vc = cache_k[:, :, :total], cache_v[:, :, :total]
    assert not kc.is_contiguous() and not q.is_contiguous()
    assert ops.decode_attn_ok(q, kc, vc)
    o, lse = ext.attn_decode(q, kc, vc, case.scale, None,
                             case.kv_lens.cuda())
    assert _same_bits((o.cpu(), lse.cpu()), want)
    # the public op reads the same views
    o2 = ops.flash_attention_decode(q, kc, vc, case.kv_lens.cuda(),
                                    case.scale)
    assert torch.equal(_bits(o2.cpu()), _bits(want[0]))


# ---------------------------------------------------------------- routing

@pytest.fixture()
def decode_mode(monkeypatch):
    from alpa_amd.global_env import global_config

    def set_mode(mode):
        monkeypatch.setattr(global_config, "decode_attention", mode)
    return set_mode


def test_env_variable_sets_the_mode(monkeypatch):
    from alpa_amd.global_env import GlobalConfig
    monkeypatch.setenv("ALPA_AMD_DECODE_ATTN", "0")
    assert GlobalConfig().decode_attention == "0"
    monkeypatch.delenv("ALPA_AMD_DECODE_ATTN")
    assert GlobalConfig().decode_attention == "auto"


def test_varlen_routes_wide_heads(ext, decode_mode):
    """flash_attention_varlen at head_dim 256: the decode kernel's result
    where it used to raise; with the mode off it raises again."""
    D = 256
    C = ops.DECODE_ATTN_CHUNK(D)
    case = DC.random_case(C + 1, D, False, (C + 1, 7))
    q, k, v, lens = (t.cuda() for t in (case.q, case.k, case.v,
                                        case.kv_lens))
    decode_mode("1")
    o = ops.flash_attention_varlen(q, k, v, lens)
    want, _ = ext.attn_decode(q, k, v, case.scale, None, lens)
    assert torch.equal(_bits(o), _bits(want))
    decode_mode("0")
    with pytest.raises(NotImplementedError):
        ops.flash_attention_varlen(q, k, v, lens)


def test_varlen_routes_narrow_heads(ext, decode_mode):
    D = 64
    case = DC.random_case(70, D, False, (70, 33))
    q, k, v, lens = (t.cuda() for t in (case.q, case.k, case.v,
                                        case.kv_lens))
    decode_mode("1")
    o = ops.flash_attention_varlen(q, k, v, lens)
    want, _ = ext.attn_decode(q, k, v, case.scale, None, lens)
    assert torch.equal(_bits(o), _bits(want))
    decode_mode("0")
    o = ops.flash_attention_varlen(q, k, v, lens)
    old, _ = ext.attn_fwd(q, k, v, False, case.scale, None, lens)
    assert torch.equal(_bits(o), _bits(old))


@pytest.mark.parametrize("D,alibi", [(64, False), (128, True), (256, False)])
def test_flash_attention_routes_single_token(ext, decode_mode, D, alibi):
    """S_q = 1, not causal, no autograd: the decode kernel; with the mode
    off, the path it had before."""
    case = DC.random_case(130, D, alibi, None)
    q, k, v = case.q.cuda(), case.k.cuda(), case.v.cuda()
    slopes = _dev(case.alibi)
    want, _ = ext.attn_decode(q, k, v, case.scale, slopes, None)
    decode_mode("1")
    with torch.no_grad():
        o = ops.flash_attention(q, k, v, causal=False, alibi_slopes=slopes)
    assert torch.equal(_bits(o), _bits(want))
    # grad mode on but nothing requires grad: still no graph to record
    o = ops.flash_attention(q, k, v, causal=False, alibi_slopes=slopes)
    assert torch.equal(_bits(o), _bits(want))
    decode_mode("0")
    with torch.no_grad():
        o = ops.flash_attention(q, k, v, causal=False, alibi_slopes=slopes)
    if D > 128:
        old, _ = ext.attn_fwd_blocked(q, k, v, False, case.scale)
    else:
        old, _ = ext.attn_fwd(q, k, v, False, case.scale, slopes)
    assert torch.equal(_bits(o), _bits(old))


def test_flash_attention_under_autograd_is_unchanged(ext, decode_mode):
    decode_mode("1")
    case = DC.random_case(130, 64, False, None)
    q, k, v = (t.cuda().requires_grad_() for t in (case.q, case.k, case.v))
    o = ops.flash_attention(q, k, v, causal=False)
    old, _ = ext.attn_fwd(q.detach(), k.detach(), v.detach(), False,
                          case.scale)
    assert torch.equal(_bits(o.detach()), _bits(old))
    o.float().sum().backward()
    for t in (q, k, v):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())


# ---------------------------------------------------------------- capture

def test_graph_capture_with_device_lengths(ext):
    """One captured flash_attention_decode with kv_lens on the device:
    replayed after kv_lens.add_(1) it gives the eager result for the new
    lengths."""
    D = 128
    C = ops.DECODE_ATTN_CHUNK(D)
    case = DC.random_case(2 * C + 1, D, True, (C - 1, 2 * C))
    q, k, v = case.q.cuda(), case.k.cuda(), case.v.cuda()
    slopes = case.alibi.cuda()
    lens = case.kv_lens.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.flash_attention_decode(q, k, v, lens, case.scale, slopes)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = ops.flash_attention_decode(q, k, v, lens, case.scale, slopes)
    lens.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    want = ops.flash_attention_decode(q, k, v, lens.clone(), case.scale,
                                      slopes)
    assert lens.tolist() == [C, 2 * C + 1]
    assert torch.equal(_bits(o), _bits(want))
    moved = F.Case(case.q, case.k, case.v, False, case.scale, lens.cpu(),
                   case.alibi)
    o64, _, A = F.reference_fp64(moved)
    assert F.bound_ratio(o.cpu(), o64, A) <= 1.0
