"""Attention backward (gfx950 MFMA kernels) on exact integer data, through
the packed-qkv views, and on random data.

The kernels feed P and dS to the second-stage MFMAs straight from the
accumulator registers, with the contraction index permuted inside each
k = 32 step, and read the other operand with transposed LDS reads in the
matching order.  A wrong order gives errors that look plausible under a
3e-2 tolerance, so the first tests use data on which every intermediate is
exactly representable and compare bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd.ops import reference as ref

SCALE = 0.5

# (S, Skv, D, causal): every head-dim tile (64, 80 exact, 96, 128), ragged
# S, one and several blocks of 128 rows, Skv != S
EXACT_SHAPES = [
    (192, 192, 80, True),
    (130, 130, 80, True),
    (67, 67, 96, True),
    (64, 200, 80, False),
    (128, 128, 64, True),
    (128, 128, 128, True),
    (16, 16, 80, True),
]


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _ternary(gen, *shape):
    """i.i.d. values from {-1, 0, 1} as bf16 on the GPU."""
    t = torch.randint(-1, 2, shape, generator=gen, dtype=torch.int32)
    return t.to(torch.bfloat16).cuda()


def _expected(do, q, k, v, causal):
    """dq, dk, dv in fp64 for o = 0 (delta = 0), lse = 0 and S = Q K^T = 0
    (so P = 1 on every unmasked element), rounded once to bf16."""
    do, q, k, v = (t.double() for t in (do, q, k, v))
    S, Skv = q.shape[2], k.shape[2]
    assert float((q @ k.transpose(-1, -2)).abs().max()) == 0.0
    p = torch.ones(S, Skv, dtype=torch.float64, device=q.device)
    if causal:
        p = torch.tril(p)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2)) * SCALE
    dq = ds @ k
    dk = ds.transpose(-1, -2) @ q
    return tuple(t.to(torch.bfloat16) for t in (dq, dk, dv))


def _exact_inputs(S, Skv, D, zero, seed):
    B, Hh = 1, 2
    gen = torch.Generator().manual_seed(seed)
    q = _ternary(gen, B, Hh, S, D)
    k = _ternary(gen, B, Hh, Skv, D)
    v = _ternary(gen, B, Hh, Skv, D)
    do = _ternary(gen, B, Hh, S, D)
    if zero == "k":
        k.zero_()
    else:
        q.zero_()
    o = torch.zeros_like(q)
    lse = torch.zeros(B, Hh, S, device="cuda", dtype=torch.float32)
    return do, q, k, v, o, lse


@pytest.mark.parametrize("S,Skv,D,causal", EXACT_SHAPES)
def test_bwd_exact_k_zero(ext, S, Skv, D, causal):
    """K = 0: dV[kv] = sum_{q >= kv} dO[q] and dK = tril(dO V^T)^T Q / 2 show
    any q-index mismatch of the in-register P / dS operands; dQ = 0."""
    do, q, k, v, o, lse = _exact_inputs(S, Skv, D, "k", 100 + S + D)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, causal, SCALE)
    dq_e, dk_e, dv_e = _expected(do, q, k, v, causal)
    assert torch.equal(dv, dv_e)
    assert torch.equal(dk, dk_e)
    assert torch.equal(dq, dq_e)
    assert float(dq.abs().max()) == 0.0


@pytest.mark.parametrize("S,Skv,D,causal", EXACT_SHAPES)
def test_bwd_exact_q_zero(ext, S, Skv, D, causal):
    """Q = 0: dQ = tril(dO V^T) K / 2 shows any kv-index mismatch in the dq
    kernel; dK = 0."""
    do, q, k, v, o, lse = _exact_inputs(S, Skv, D, "q", 200 + S + D)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, causal, SCALE)
    dq_e, dk_e, dv_e = _expected(do, q, k, v, causal)
    assert torch.equal(dq, dq_e)
    assert torch.equal(dv, dv_e)
    assert torch.equal(dk, dk_e)
    assert float(dk.abs().max()) == 0.0


def test_bwd_exact_packed_views(ext):
    """Case K = 0 through the packed layout: q/k/v are strided views of one
    [B, S, h*3*d] buffer, dq/dk/dv views of one NaN-filled dqkv buffer."""
    from alpa_amd.ops import _qkv_views
    B, S, h, d = 1, 130, 2, 80
    gen = torch.Generator().manual_seed(7)
    qkv = _ternary(gen, B, S, h * 3 * d)
    q, k, v = _qkv_views(qkv, h)
    k.zero_()
    do_buf = _ternary(gen, B, S, h * d)
    o_buf = torch.zeros_like(do_buf)
    do4 = do_buf.view(B, S, h, d).permute(0, 2, 1, 3)
    o4 = o_buf.view(B, S, h, d).permute(0, 2, 1, 3)
    lse = torch.zeros(B, h, S, device="cuda", dtype=torch.float32)
    dqkv = torch.full_like(qkv, float("nan"))
    dq_v, dk_v, dv_v = _qkv_views(dqkv, h)
    ext.attn_bwd_out(do4, q, k, v, o4, lse, dq_v, dk_v, dv_v, True, SCALE)
    dq_e, dk_e, dv_e = _expected(do4, q, k, v, True)
    assert not bool(torch.isnan(dqkv).any())
    assert torch.equal(dq_v, dq_e)
    assert torch.equal(dk_v, dk_e)
    assert torch.equal(dv_v, dv_e)


@pytest.mark.parametrize("S,Skv,D,causal,alibi", [
    (192, 192, 80, True, False),
    (130, 130, 80, True, True),
    (67, 67, 96, True, False),
    (64, 200, 80, False, False),
])
def test_bwd_random_vs_reference(ext, S, Skv, D, causal, alibi):
    """randn inputs against the fp32 reference, and run-to-run determinism."""
    torch.manual_seed(21)
    B, Hh = 1, 2
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    slopes = (torch.tensor([0.25, 0.0625], device="cuda")
              if alibi else None)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, causal, scale, slopes)
    lse3 = lse.view(B, Hh, S)
    do = torch.randn_like(o)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse3, causal, scale, slopes)
    dq2, dk2, dv2 = ext.attn_bwd(do, q, k, v, o, lse3, causal, scale, slopes)
    assert torch.equal(dq, dq2)
    assert torch.equal(dk, dk2)
    assert torch.equal(dv, dv2)
    dq_r, dk_r, dv_r = ref.attention_bwd(do.float(), q.float(), k.float(),
                                         v.float(), o.float(), lse3, causal,
                                         scale, slopes)
    torch.testing.assert_close(dq.float(), dq_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk.float(), dk_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv.float(), dv_r, rtol=3e-2, atol=3e-2)
