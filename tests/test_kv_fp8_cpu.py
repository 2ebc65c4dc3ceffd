"""The e4m3 KV cache without a GPU: the row format of ops.reference, the cache
container, and a decoder that runs through the reference path."""
import pytest
import torch

import kv_fp8_cases as KC
from alpa_amd import ops
from alpa_amd.global_env import global_config
from alpa_amd.models.decoder import KVCache
from alpa_amd.ops import reference as ref


def test_rows_round_trip():
    torch.manual_seed(1)
    x = (torch.randn(4, 3, 7, 80) *
         torch.exp2(torch.randint(-12, 12, (4, 3, 7, 1)).float())).bfloat16()
    x[0, 0, 0] = 0
    q, scale = ref.kv_quantize_rows(x)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    KC.check_rows(x, q, scale)
    assert torch.equal(ref.kv_dequantize_rows(q, scale),
                       q.float() * scale.unsqueeze(-1))


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_non_finite_row_is_not_clamped(poison):
    x = torch.randn(3, 32).bfloat16()
    x[1, 5] = poison
    q, scale = ref.kv_quantize_rows(x)
    d = ref.kv_dequantize_rows(q, scale)
    assert bool(torch.isnan(d[1]).all()) and bool(torch.isfinite(d[[0, 2]]).all())
    assert bool((q.view(torch.uint8)[1] == 0x7F).all())


def test_cache_container(monkeypatch):
    m = KC.tiny_model("bloom", torch.float32, "cpu")
    off = m.new_cache(2, max_len=8)
    assert not off.fp8 and off.k_scale is None and off.v_scale is None
    assert all(t.dtype == torch.float32 and t.shape == (2, 2, 8, 64)
               for t in off.k + off.v)
    monkeypatch.setattr(global_config, "kv_cache_fp8", True)
    on = m.new_cache(3, max_len=8)
    assert on.k[0].dtype == torch.float8_e4m3fn
    assert on.k_scale[1].shape == (3, 2, 8)
    for ts in (on.k, on.v):
        for t in ts:
            t.view(torch.uint8)[:] = torch.arange(3).view(3, 1, 1, 1)
    for ts in (on.k_scale, on.v_scale):
        for t in ts:
            t[:] = torch.arange(3.).view(3, 1, 1)
    on.reorder(torch.tensor([2, 0, 0]))
    for ts in (on.k, on.v):
        assert ts[1].view(torch.uint8)[:, 0, 0, 0].tolist() == [2, 0, 0]
    for ts in (on.k_scale, on.v_scale):
        assert ts[1][:, 0, 0].tolist() == [2., 0., 0.]


@pytest.mark.parametrize("name", ["codegen", "bloom"])
def test_cpu_model_decodes_through_the_reference(monkeypatch, name):
    """Prefill, then one cached step over the reference e4m3 cache, against
    the model's own full forward.  This is the measurement behind
    kv_fp8_cases.EFFECT; it may move by no more than its own size."""
    monkeypatch.setattr(global_config, "kv_cache_fp8", True)
    inc, full = KC.cached_step_and_full(
        KC.tiny_model(name, torch.float32, "cpu"), name)
    err = float((inc - full).abs().max())
    print(f"{name}: e4m3 cache effect {err:.4f}")
    assert 0 < err <= 2 * KC.EFFECT[name]
