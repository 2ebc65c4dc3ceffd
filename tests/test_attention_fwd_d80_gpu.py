"""Attention forward at D = 80, which has its own instantiation (rows of
exactly 80 elements, 5 output d-tiles, a half-zero third k step), and at
shapes that exercise waves of two 16-row sets: the exact families of
test_attention_fwd_exact_gpu.py (attn_fwd_cases.py) at the shapes of
attn_fwd_d80_shapes.py, plus run-to-run determinism."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_fwd_cases as C
import attn_fwd_d80_shapes as SH


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _run(ext, case):
    """(o, lse) of the kernel, back on the CPU."""
    dev = lambda t: None if t is None else t.cuda()
    o, lse = ext.attn_fwd(dev(case.q), dev(case.k), dev(case.v), case.causal,
                          case.scale, dev(case.alibi), dev(case.kv_lens))
    assert lse.shape == case.q.shape[:3] and lse.dtype == torch.float32
    return o.cpu(), lse.cpu()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


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
    o64, lse64, A = C.reference_fp64(case)
    ratio = C.bound_ratio(o, o64, A)
    lse_err = float((lse.double() - lse64).abs().max())
    print(f"err/bound {ratio:.3f}  lse err {lse_err:.3g}")
    assert ratio <= 1.0
    torch.testing.assert_close(lse.double(), lse64, rtol=0, atol=C.LSE_ATOL)


@pytest.mark.parametrize("S,Skv,D,causal", SH.AB_SHAPES)
def test_fwd_one_hot(ext, S, Skv, D, causal):
    case = C.one_hot(S, Skv, D, causal)
    o, lse = _run(ext, case)
    assert torch.equal(lse, case.lse)
    assert torch.equal(o, case.o)


@pytest.mark.parametrize("S,Skv,D,causal", SH.AB_SHAPES)
def test_fwd_uniform(ext, S, Skv, D, causal):
    case = C.uniform(S, Skv, D, causal)
    _check_uniform(*_run(ext, case), case)


@pytest.mark.parametrize("S,d,causal", SH.VIEW_SHAPES)
def test_fwd_one_hot_packed_views(ext, S, d, causal):
    """q, k, v as strided views of one packed buffer, o as a view of a wider
    buffer: every o[..., :d] and lse entry is written, 8 bytes at a time,
    and the 16 padding columns next to each row keep their sentinel."""
    from alpa_amd.ops import _qkv_views
    case = C.one_hot(S, S, d, causal)
    qkv = torch.empty(C.B, S, C.H * 3 * d, dtype=torch.bfloat16,
                      device="cuda")
    q, k, v = _qkv_views(qkv, C.H)
    q.copy_(case.q)
    k.copy_(case.k)
    v.copy_(case.v)
    assert not q.is_contiguous() and q.stride(3) == 1
    sentinel = 0x5A5A
    o_buf = torch.full((C.B, S, C.H, d + 16), sentinel, dtype=torch.int16,
                       device="cuda").view(torch.bfloat16)
    o_view = o_buf[..., :d].permute(0, 2, 1, 3)
    lse = torch.full((C.B, C.H, S), math.nan, dtype=torch.float32,
                     device="cuda")
    ext.attn_fwd_out(q, k, v, o_view, lse, causal, case.scale)
    assert torch.equal(lse.cpu(), case.lse)
    assert torch.equal(o_view.cpu(), case.o)
    assert bool((_bits(o_buf)[..., d:] == sentinel).all())


def test_fwd_one_hot_unaligned_o_rows(ext):
    """o rows that start on odd elements (one padding column per head) take
    the 2-byte stores: same values, and the padding column is intact."""
    S, d, causal = SH.VIEW_SHAPES[1]
    case = C.one_hot(S, S, d, causal)
    sentinel = 0x5A5A
    o_buf = torch.full((C.B, S, C.H, d + 1), sentinel, dtype=torch.int16,
                       device="cuda").view(torch.bfloat16)
    o_view = o_buf[..., :d].permute(0, 2, 1, 3)
    assert o_view.stride(1) % 4 != 0
    lse = torch.full((C.B, C.H, S), math.nan, dtype=torch.float32,
                     device="cuda")
    ext.attn_fwd_out(case.q.cuda(), case.k.cuda(), case.v.cuda(), o_view,
                     lse, causal, case.scale)
    assert torch.equal(lse.cpu(), case.lse)
    assert torch.equal(o_view.cpu(), case.o)
    assert bool((_bits(o_buf)[..., d:] == sentinel).all())


@pytest.mark.parametrize("S,Skv,D,causal,order", SH.STAIR_SHAPES)
def test_fwd_staircase(ext, S, Skv, D, causal, order):
    case = C.staircase(S, Skv, D, causal, order)
    _check_fp64(*_run(ext, case), case)


@pytest.mark.parametrize("S,Skv,D,causal,alibi,kv_lens", SH.RANDOM_SHAPES)
def test_fwd_random(ext, S, Skv, D, causal, alibi, kv_lens):
    case = C.random_case(S, Skv, D, causal, alibi, kv_lens)
    _check_fp64(*_run(ext, case), case)


def test_fwd_tail_is_ignored(ext):
    """NaN in k and in v at and past kv_lens[b] gives the bits of the
    unpoisoned run."""
    S, Skv, D, kv_lens = SH.TAIL_SHAPE
    case = C.uniform(S, Skv, D, False, kv_lens)
    o0, lse0 = _run(ext, case)
    bad = C.poison_tail(C.poison_tail(case, "k", math.nan), "v", math.nan)
    o, lse = _run(ext, bad)
    assert torch.equal(_bits(lse), _bits(lse0))
    assert torch.equal(_bits(o), _bits(o0))
    _check_uniform(o, lse, case)


def test_fwd_is_deterministic(ext):
    """Two runs give the same bits (mfma_f32_16x16x16bf16_1k in the tail
    step of the contraction over d did not, see attention_bwd.hip)."""
    case = C.random_case(*SH.DETERMINISM_SHAPE)
    o, lse = _run(ext, case)
    o2, lse2 = _run(ext, case)
    assert torch.equal(_bits(o), _bits(o2))
    assert torch.equal(_bits(lse), _bits(lse2))
