"""MFMA skinny GEMM (csrc/skinny_mfma.hip, 9..64 tokens) against fp64
references: exact on integer data, per-element bound on realistic data,
layer routing, and the binding's refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(128, 512), (192, 768)]  # legal splits {1, 2} and {1, 3}


def _mfma(w, x, scale, bias, splits):
    """w [N, K]: bf16, or e4m3 together with its scale; packed to the
    kernels' [K/8, N, 8] layout."""
    from alpa_amd.ops._backend import hip_ops
    N, K = w.shape
    ws = None
    if w.dtype == torch.float8_e4m3fn:
        w, ws = w.view(torch.uint8), torch.tensor([scale], device="cuda")
    wp = w.view(N, K // 8, 8).permute(1, 0, 2).contiguous()
    return hip_ops().skinny_gemm_mfma(wp, x, ws, bias, N, K, splits)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [9, 16, 17, 33, 64])
def test_exact_on_integers(M, N, K, fp8, bias):
    """Integers in -2..2 (e4m3 scale 0.5): every product and partial sum is
    exact in fp32 in any order, so the result is the fp64 one rounded once,
    whatever the split."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    x = torch.randint(-2, 3, (M, K), generator=g).cuda().to(torch.bfloat16)
    w = torch.randint(-2, 3, (N, K), generator=g).cuda().to(torch.bfloat16)
    b = torch.randint(-2, 3, (N,), generator=g).cuda().to(torch.bfloat16) \
        if bias else None
    scale = 0.5 if fp8 else 1.0
    want = x.double() @ w.double().t() * scale
    if bias:
        want = want + b.double()
    want = want.to(torch.bfloat16)
    if fp8:
        w = w.to(torch.float8_e4m3fn)
    for splits in (1, K // 256):  # fused epilogue, partials + finalize
        got = _mfma(w, x, scale, b, splits)
        assert torch.equal(got, want), (splits, (got != want).sum().item())


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [9, 64])
def test_realistic_magnitudes(M, N, K, fp8):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |w|^T) per element: one bf16
    rounding (with slack for a double rounding) plus the fp32 accumulation
    bound; ref is fp64 on the weights the kernel sees."""
    torch.manual_seed(M + N)
    x = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") * 0.05).to(torch.bfloat16)
    scale = 1.0
    if fp8:
        # the float the kernel reads, so that ref uses the same factor
        scale = (w.abs().amax().float() / 448.0).item()
        w = (w.float() / scale).to(torch.float8_e4m3fn)
    wd = w.float().double() * scale
    ref = x.double() @ wd.t()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs()
                                                      @ wd.abs().t())
    for splits in (1, K // 256):
        err = (_mfma(w, x, scale, None, splits).double() - ref).abs()
        worst = (err / bound).max().item()
        print(f"M={M} N={N} K={K} fp8={fp8} S={splits}: err/bound {worst:.3f}")
        assert (err <= bound).all(), worst


def test_layers_route_by_token_count():
    from alpa_amd import ops
    from alpa_amd.global_env import global_config
    from alpa_amd.ops._backend import hip_ops
    from alpa_amd.parallel.layers import (ColumnParallelLinear,
                                          RowParallelLinear)
    kw = dict(bias=False, dtype=torch.bfloat16, device=torch.device("cuda"),
              init_seed=0, init_tag="t")
    torch.manual_seed(0)
    x16 = (torch.randn(16, 1, 512, device="cuda") * 0.5).to(torch.bfloat16)
    x4 = x16[:4].contiguous()
    old = global_config.skinny_gemm
    try:
        with torch.no_grad():
            for cls in (ColumnParallelLinear, RowParallelLinear):
                global_config.skinny_gemm = "0"
                lin = cls(512, 640, None, 1, **kw)
                lin(x16)
                assert not hasattr(lin, "_skinny_pack")
                global_config.skinny_gemm = "1"
                y16, y4 = lin(x16), lin(x4)
                wp = lin._skinny_pack[1]
                s16 = ops._SKINNY_TUNED[(640, 512, 16, False, "mfma")]
                s4 = ops._SKINNY_TUNED[(640, 512, 4, False, "dot2")]
                d16 = hip_ops().skinny_gemm_mfma(wp, x16.view(16, 512), None,
                                                 None, 640, 512, s16)
                d4 = hip_ops().skinny_gemm(wp, x4.view(4, 512), None, None,
                                           640, 512, s4)
                assert torch.equal(y16.view(16, 640), d16)
                assert torch.equal(y4.view(4, 640), d4)
    finally:
        global_config.skinny_gemm = old


def _operands(M=16, N=128, K=512, xdtype=torch.bfloat16):
    return dict(wp=torch.zeros(K // 8, N, 8, device="cuda",
                               dtype=torch.bfloat16),
                x=torch.zeros(M, K, device="cuda", dtype=xdtype),
                wscale=None, bias=None, N=N, K=K, splits=1)


@pytest.mark.parametrize("name,change", [
    ("N", lambda: _operands(N=96)),
    ("K", lambda: _operands(K=320)),
    ("splits", lambda: dict(_operands(), splits=0)),
    ("splits", lambda: dict(_operands(K=768), splits=2)),
    ("x", lambda: _operands(M=65)),
    ("x", lambda: _operands(M=0)),
    ("x", lambda: _operands(xdtype=torch.float32)),
    ("wp", lambda: dict(_operands(), wscale=torch.ones(1, device="cuda"))),
    ("bias", lambda: dict(_operands(), bias=torch.zeros(
        64, device="cuda", dtype=torch.bfloat16))),
], ids=["N96", "K320", "splits0", "split_not_dividing", "M65", "empty_x",
        "fp32_x", "wscale_with_bf16_wp", "short_bias"])
def test_refusals_name_the_operand(name, change):
    from alpa_amd.ops._backend import hip_ops
    a = change()
    with pytest.raises(RuntimeError) as e:
        hip_ops().skinny_gemm_mfma(a["wp"], a["x"], a["wscale"], a["bias"],
                                   a["N"], a["K"], a["splits"])
    assert name in str(e.value) and "HIP error" not in str(e.value)
