"""Attention forward (gfx950 MFMA kernel) on inputs with exactly known
outputs, at edge shapes, through strided views and with poisoned memory
past kv_lens.

The randn tests in test_kernels_gpu.py never take the deferred online-softmax
rescale after the first kv tile, and their atol of 2e-2 is larger than the
effect of a dropped V tile.  The families used here (attn_fwd_cases.py):

  A one-hot    o = v[pi] and lse = 64 D bit for bit: key and value indexing,
               the V transpose, head-dim columns, the LDS buffer, and the
               rescale with alpha = 0
  B uniform    o = bf16(sum of visible v / n) bit for bit, lse = log n:
               masks and counts
  C staircase  the wave-wide rescale with 0 < alpha < 1, against fp64
  D random     ALiBi with kv_lens and the remaining feature combinations,
               against fp64

C and D use the derived bound |o - o_ref64| <= 2^-7 * (P @ |V|) + 1e-6."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_fwd_cases as C


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


@pytest.mark.parametrize("S,Skv,D,causal", C.AB_SHAPES)
def test_fwd_one_hot(ext, S, Skv, D, causal):
    case = C.one_hot(S, Skv, D, causal)
    o, lse = _run(ext, case)
    assert torch.equal(lse, case.lse)
    assert torch.equal(o, case.o)


@pytest.mark.parametrize("S,Skv,D,kv_lens", C.VARLEN_SHAPES)
def test_fwd_one_hot_varlen(ext, S, Skv, D, kv_lens):
    """An empty slot gives o = 0 and lse = -inf."""
    case = C.one_hot(S, Skv, D, False, kv_lens)
    o, lse = _run(ext, case)
    assert torch.equal(lse, case.lse)
    assert torch.equal(o, case.o)


@pytest.mark.parametrize("S,Skv,D,causal", C.AB_SHAPES + C.B_ONLY_SHAPES)
def test_fwd_uniform(ext, S, Skv, D, causal):
    case = C.uniform(S, Skv, D, causal)
    _check_uniform(*_run(ext, case), case)


@pytest.mark.parametrize("S,Skv,D,kv_lens",
                         C.VARLEN_SHAPES + C.B_ONLY_VARLEN_SHAPES)
def test_fwd_uniform_varlen(ext, S, Skv, D, kv_lens):
    case = C.uniform(S, Skv, D, False, kv_lens)
    _check_uniform(*_run(ext, case), case)


@pytest.mark.parametrize("S,d,causal", C.VIEW_SHAPES)
def test_fwd_one_hot_packed_views(ext, S, d, causal):
    """q, k, v as strided views of one packed buffer, o as a view of a wider
    buffer: every o[..., :d] and lse entry is written, and the 16 padding
    columns next to each row keep their sentinel."""
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


@pytest.mark.parametrize("S,Skv,D,causal,order", C.STAIR_SHAPES)
def test_fwd_staircase(ext, S, Skv, D, causal, order):
    """Measured err/bound on MI355X: 0.23 to 0.91, equal to the CPU
    emulation's figure in every case.  The two largest, 0.909 at
    (200, 200, 96, causal, asc) and 0.903 at (130, 257, 128, full, asc), are
    rows with g = 9 in which one key holds p = 0.97 to 0.99: nothing
    averages, and the bf16 rounding of that P and the bf16 rounding of o
    both fall near half an ulp with the same sign."""
    case = C.staircase(S, Skv, D, causal, order)
    o, lse = _run(ext, case)
    o2, lse2 = _run(ext, case)
    assert torch.equal(_bits(o), _bits(o2))
    assert torch.equal(_bits(lse), _bits(lse2))
    _check_fp64(o, lse, case)


@pytest.mark.parametrize("S,Skv,D,causal,alibi,kv_lens", C.RANDOM_SHAPES)
def test_fwd_random(ext, S, Skv, D, causal, alibi, kv_lens):
    case = C.random_case(S, Skv, D, causal, alibi, kv_lens)
    _check_fp64(*_run(ext, case), case)


@pytest.mark.parametrize("value", [math.nan, math.inf])
@pytest.mark.parametrize("which", ["v", "k"])
@pytest.mark.parametrize("S,Skv,D,kv_lens", C.TAIL_SHAPES)
def test_fwd_tail_is_ignored(ext, S, Skv, D, kv_lens, which, value):
    """Memory at and past kv_lens[b] is never observed: NaN or Inf there
    gives the same bits as zeros."""
    case = C.uniform(S, Skv, D, False, kv_lens)
    o0, lse0 = _run(ext, C.poison_tail(case, which, 0.0))
    o, lse = _run(ext, C.poison_tail(case, which, value))
    assert torch.equal(_bits(lse), _bits(lse0))
    assert torch.equal(_bits(o), _bits(o0))
    _check_uniform(o, lse, case)
