"""MXFP4 decode kernels (csrc/skinny_fp4.hip up to 8 tokens,
csrc/skinny_mfma_fp4.hip for 9..64) against fp64 on the dequantized weights:
exact on integer data, per-element bound on realistic data, the quantizer on
both devices, layer routing under global_config.weight_fp4, refusals."""
import functools

import pytest
import torch

import mxfp4_cases as MC

pytestmark = pytest.mark.gpu

SHAPES = [(128, 512), (192, 768)]  # legal splits {1, 2} and {1, 3}
DOT2_M, MFMA_M = [1, 4, 5, 8], [9, 16, 17, 33, 64]


def _gemm(codes, scales, x, bias, splits):
    """The binding that serves x's token count, on freshly packed weights."""
    from alpa_amd import ops
    from alpa_amd.ops._backend import hip_ops
    N, K = scales.shape[0], scales.shape[1] * 32
    wq, sq = ops.mxfp4_pack(codes, scales)
    f = hip_ops().skinny_gemm_fp4 if x.shape[0] <= 8 \
        else hip_ops().skinny_gemm_mfma_fp4
    return f(wq, sq, x, bias, N, K, splits)


@functools.lru_cache(maxsize=None)
def _integer_case(N, K):
    """Weights straight from codes and scales (every code, scales 1/2, 1, 2
    by row and block), x and bias integers in -2..2: every product is a
    multiple of 1/4 and every partial sum stays below 2^15, exact in fp32 in
    any order."""
    from alpa_amd import ops
    codes, scales = MC.all_codes(N, K, seed=N)
    g = torch.Generator().manual_seed(K)
    x = torch.randint(-2, 3, (64, K), generator=g).cuda().to(torch.bfloat16)
    b = torch.randint(-2, 3, (N,), generator=g).cuda().to(torch.bfloat16)
    codes, scales = codes.cuda(), scales.cuda()
    w = ops.mxfp4_dequantize(codes, scales, torch.float32).double()
    return codes, scales, x, b, x.double() @ w.t()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", DOT2_M + MFMA_M)
def test_exact_on_integers(M, N, K, bias):
    codes, scales, x, b, ref = _integer_case(N, K)
    want = (ref[:M] + b.double() if bias else ref[:M]).to(torch.bfloat16)
    for splits in (1, K // 256):
        got = _gemm(codes, scales, x[:M], b if bias else None, splits)
        assert torch.equal(got, want), (splits, (got != want).sum().item())


@functools.lru_cache(maxsize=None)
def _realistic_case(N, K):
    from alpa_amd import ops
    torch.manual_seed(N)
    x = (torch.randn(64, K, device="cuda") * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") * 0.05).to(torch.bfloat16)
    codes, scales = ops.mxfp4_quantize(w)
    wd = ops.mxfp4_dequantize(codes, scales).double()
    return codes, scales, x, x.double() @ wd.t(), x.double().abs() @ wd.abs().t()


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 8, 9, 64])
def test_realistic_magnitudes(M, N, K):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |w_deq|^T) per element, the
    bound of tests/test_skinny_mfma_gpu.py: one bf16 rounding (with slack for
    a double rounding) plus the fp32 accumulation bound; ref is fp64 on the
    dequantized weights, which are what the kernels multiply."""
    codes, scales, x, ref, mag = _realistic_case(N, K)
    bound = 2.0 ** -8 * ref[:M].abs() + K * 2.0 ** -23 * mag[:M]
    for splits in (1, K // 256):
        err = (_gemm(codes, scales, x[:M], None, splits).double()
               - ref[:M]).abs()
        worst = (err / bound).max().item()
        print(f"M={M} N={N} K={K} S={splits}: err/bound {worst:.3f}")
        assert (err <= bound).all(), worst


def test_quantizer_agrees_across_devices():
    from alpa_amd import ops
    w, scales, codes = MC.rows()
    got_codes, got_scales = ops.mxfp4_quantize(w.cuda())
    assert torch.equal(got_codes.cpu(), codes)
    assert torch.equal(got_scales.cpu(), scales)
    for dtype in (torch.bfloat16, torch.float32):
        assert torch.equal(ops.mxfp4_dequantize(codes.cuda(), scales.cuda(),
                                                dtype).cpu(),
                           ops.mxfp4_dequantize(codes, scales, dtype))
    torch.manual_seed(0)
    r = (torch.randn(64, 256) * 0.05).to(torch.bfloat16)
    for a, b in zip(ops.mxfp4_quantize(r.cuda()), ops.mxfp4_quantize(r)):
        assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("cls", ["ColumnParallelLinear", "RowParallelLinear"])
def test_layers_route_by_flag(cls):
    from alpa_amd import ops
    from alpa_amd.global_env import global_config
    from alpa_amd.ops._backend import hip_ops
    from alpa_amd.parallel import layers
    kw = dict(bias=False, dtype=torch.bfloat16, device=torch.device("cuda"),
              init_seed=0, init_tag="t")
    torch.manual_seed(0)
    x16 = (torch.randn(16, 1, 512, device="cuda") * 0.5).to(torch.bfloat16)
    x4 = x16[:4].contiguous()
    old = global_config.skinny_gemm, global_config.weight_fp4
    try:
        global_config.skinny_gemm = "1"
        with torch.no_grad():
            a, b, head = (getattr(layers, cls)(512, 640, None, 1, **kw)
                          for _ in range(3))
            head._fp8_exclude = True
            global_config.weight_fp4 = True
            y16, y4, h_on = a(x16), a(x4), head(x16)
            key, wq, sq = a._skinny_pack
            assert key[1] == "mxfp4" and wq.dtype == torch.uint8
            s16 = ops._SKINNY_TUNED[(640, 512, 16, "mxfp4", "mfma")]
            s4 = ops._SKINNY_TUNED[(640, 512, 4, "mxfp4", "dot2")]
            d16 = hip_ops().skinny_gemm_mfma_fp4(wq, sq, x16.view(16, 512),
                                                 None, 640, 512, s16)
            d4 = hip_ops().skinny_gemm_fp4(wq, sq, x4.view(4, 512), None,
                                           640, 512, s4)
            assert torch.equal(y16.view(16, 640), d16)
            assert torch.equal(y4.view(4, 640), d4)
            assert head._skinny_pack[1].dtype == torch.bfloat16
            global_config.weight_fp4 = False
            # a's fp4 pack is stale under the new format and is replaced
            for x in (x16, x4):
                assert torch.equal(a(x), b(x))
            assert torch.equal(head(x16), h_on)
            for lin in (a, b):
                assert lin._skinny_pack[0][1] != "mxfp4"
                assert lin._skinny_pack[1].dtype == torch.bfloat16
    finally:
        global_config.skinny_gemm, global_config.weight_fp4 = old


def _operands(M, N=128, K=512):
    return dict(wq=torch.zeros(K // 32, N, 16, device="cuda",
                               dtype=torch.uint8),
                sq=torch.zeros(K // 256, N, 8, device="cuda",
                               dtype=torch.uint8),
                x=torch.zeros(M, K, device="cuda", dtype=torch.bfloat16),
                bias=None, N=N, K=K, splits=1)


@pytest.mark.parametrize("binding,M,too_many", [
    ("skinny_gemm_fp4", 4, 9), ("skinny_gemm_mfma_fp4", 16, 65)])
@pytest.mark.parametrize("name,change", [
    ("sq", lambda M: dict(_operands(M), sq=torch.zeros(
        128, 512 // 32, device="cuda", dtype=torch.uint8))),
    ("K", lambda M: _operands(M, K=272)),
    ("splits", lambda M: dict(_operands(M, K=768), splits=2)),
    ("x", None),
], ids=["scales_shape", "K_not_whole_blocks", "split_not_dividing",
        "M_out_of_range"])
def test_refusals_name_the_operand(binding, M, too_many, name, change):
    from alpa_amd.ops._backend import hip_ops
    a = change(M) if change else _operands(too_many)
    with pytest.raises(RuntimeError) as e:
        getattr(hip_ops(), binding)(a["wq"], a["sq"], a["x"], a["bias"],
                                    a["N"], a["K"], a["splits"])
    assert name in str(e.value) and "HIP error" not in str(e.value)
