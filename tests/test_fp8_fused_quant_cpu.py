"""Reference (CPU) side of the producer-fused fp8 quantize: the two
reference ops against the hand-composed LayerNorm / GeLU reference plus
cast, and the public entry points' dispatch on CPU tensors."""
import pytest
import torch

from alpa_amd.ops import reference as ref

SHAPES = [(100, 200), (1, 8)]


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, f = shape
    x = (torch.randn(n, f, generator=g) * 3).to(torch.bfloat16)
    d = torch.randn(n, f, generator=g).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(f, generator=g)).to(torch.bfloat16)
    b = (0.1 * torch.randn(f, generator=g)).to(torch.bfloat16)
    return x, d, w, b, torch.tensor([0.02])


def _cast(y, scale):
    return (y.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)


def _check_quant(q, qt, amax, y, scale):
    want = _cast(y, scale)
    assert q.dtype == torch.float8_e4m3fn and q.shape == y.shape
    assert torch.equal(q.view(torch.uint8), want.view(torch.uint8))
    assert qt.shape == (y.shape[1], y.shape[0]) and qt.is_contiguous()
    assert torch.equal(qt.view(torch.uint8), q.t().view(torch.uint8))
    assert amax.dtype == torch.float32 and amax.shape == (1,)
    assert amax.item() == y.float().abs().max().item()


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_bias_gelu_fp8(shape):
    x, _, _, b, scale = _inputs(shape, 0)
    q, qt, amax = ref.bias_gelu_fp8(x, b, scale)
    _check_quant(q, qt, amax, ref.bias_gelu_fwd(x, b), scale)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_delta", [True, False])
def test_reference_add_layer_norm_fp8(shape, with_delta):
    x, d, w, b, scale = _inputs(shape, 1)
    delta = d if with_delta else None
    h, mean, rstd, q, qt, amax = ref.add_layer_norm_fp8(x, delta, w, b, 1e-5,
                                                        scale)
    h_want = x + d if with_delta else x
    y, mean_want, rstd_want = ref.layer_norm_fwd(h_want, w, b, 1e-5)
    assert h.dtype == torch.bfloat16 and torch.equal(h, h_want)
    assert torch.equal(mean, mean_want) and torch.equal(rstd, rstd_want)
    _check_quant(q, qt, amax, y, scale)


def test_entry_points_dispatch_to_reference_on_cpu():
    """The public ops exist, are exported and run the reference on CPU
    tensors (fails before the feature: the names are missing)."""
    from alpa_amd import ops
    assert "bias_gelu_fp8" in ops.__all__
    assert "add_layer_norm_fp8" in ops.__all__
    x, d, w, b, scale = _inputs((100, 200), 2)
    for got, want in zip(ops.bias_gelu_fp8(x, b, scale),
                         ref.bias_gelu_fp8(x, b, scale)):
        assert torch.equal(got.view(torch.uint8) if got.dtype.itemsize == 1
                           else got,
                           want.view(torch.uint8) if want.dtype.itemsize == 1
                           else want)
    for delta in (d, None):
        outs = ops.add_layer_norm_fp8(x, delta, w, b, 1e-5, scale)
        wants = ref.add_layer_norm_fp8(x, delta, w, b, 1e-5, scale)
        assert len(outs) == len(wants) == 6
        for got, want in zip(outs, wants):
            assert got.dtype == want.dtype
            if got.dtype.itemsize == 1:
                got, want = got.view(torch.uint8), want.view(torch.uint8)
            assert torch.equal(got, want)
    # a 3-D input is flattened to rows, like the quantize it replaces
    q, qt, _ = ops.bias_gelu_fp8(x.view(4, 25, 200), b, scale)
    assert q.shape == (100, 200) and qt.shape == (200, 100)
    assert not q.requires_grad


def test_flag_defaults_and_env(monkeypatch):
    from alpa_amd.global_env import GlobalConfig
    monkeypatch.delenv("ALPA_AMD_FP8_FUSED_QUANT", raising=False)
    assert GlobalConfig().fp8_fused_quant is True
    monkeypatch.setenv("ALPA_AMD_FP8_FUSED_QUANT", "1")
    assert GlobalConfig().fp8_fused_quant is True
    monkeypatch.setenv("ALPA_AMD_FP8_FUSED_QUANT", "0")
    assert GlobalConfig().fp8_fused_quant is False


def test_model_untouched_outside_the_fused_route():
    """fp8_gemm on a CPU model: no linear qualifies for fp8, so with the
    flag on the block threads (res, delta, ln) and the deferred GeLU
    through the layers and every one of them falls back to the unfused
    ops: same loss and gradients as with the flag off."""
    from alpa_amd.global_env import global_config
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    cfg = GPTConfig(hidden_size=32, num_layers=2, num_heads=2, seq_len=16,
                    vocab_size=64)
    ids = torch.randint(0, 64, (2, 16), generator=torch.Generator()
                        .manual_seed(0))
    old = (global_config.fp8_fused_quant, global_config.fp8_gemm)
    losses = []
    try:
        global_config.fp8_gemm = True
        for flag in (False, True):
            global_config.fp8_fused_quant = flag
            m = GPTModel(cfg, None, 1, torch.float32, None, init_seed=3)
            loss = m.loss(ids, ids)
            loss.backward()
            losses.append((loss.item(),
                           m.blocks[0].mlp.fc1.weight.grad.clone()))
    finally:
        global_config.fp8_fused_quant, global_config.fp8_gemm = old
    assert losses[0][0] == losses[1][0]
    assert torch.equal(losses[0][1], losses[1][1])
