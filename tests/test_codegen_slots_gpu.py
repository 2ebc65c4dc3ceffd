"""CodeGen at per-slot positions: ops.qkv_cache_write rotates q and k at
positions it reads on the device, which is what forward_decode (continuous
batching) and the captured decode loop need.  The tiny CodeGen of
kv_fp8_cases, bf16, over a bf16 and an e4m3 cache."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import kv_fp8_cases as KC
from alpa_amd.global_env import global_config


@pytest.fixture(params=[False, True], ids=["bf16", "e4m3"])
def model(request, monkeypatch):
    monkeypatch.setattr(global_config, "kv_cache_fp8", request.param)
    return KC.tiny_model("codegen", torch.bfloat16, "cuda")


def _ids(*shape):
    gen = torch.Generator().manual_seed(sum(shape))
    return torch.randint(0, KC.VOCAB["codegen"], shape, generator=gen).cuda()


@torch.no_grad()
def test_decode_at_equal_lens_is_the_common_step(model):
    """Both go through the same kernels, whose bits do not depend on how the
    position arrives."""
    n = 7
    cache = model.new_cache(2, max_len=16)
    model.forward_step(_ids(2, n), cache)
    twin, tok = copy.deepcopy(cache), _ids(2, 1)
    lens = torch.full((2,), n, device="cuda")
    assert torch.equal(model.forward_decode(tok, cache, lens),
                       model.forward_step(tok, twin))


@torch.no_grad()
def test_decode_at_unequal_lens(model):
    """Slots of 5 and 9 tokens, prefilled through cache.slots, against each
    slot decoded alone.  Tolerance: the 5e-2 of cached-versus-full in bf16,
    plus twice the measured effect of the e4m3 cache on that cache."""
    lens, tok = [5, 9], _ids(2, 1)
    cache = model.new_cache(2, max_len=16)
    alone = []
    for b, n in enumerate(lens):
        ids = _ids(1, n)
        model.forward_step(ids, cache.slots(b, 1))
        solo = model.new_cache(1, max_len=16)
        model.forward_step(ids, solo)
        alone.append(model.forward_step(tok[b:b + 1], solo))
    got = model.forward_decode(tok, cache, torch.tensor(lens, device="cuda"))
    atol = 5e-2 + (2 * KC.EFFECT["codegen"] if cache.fp8 else 0.0)
    print("max |batched - alone|",
          float((got.float() - torch.cat(alone).float()).abs().max()))
    torch.testing.assert_close(got.float(), torch.cat(alone).float(),
                               rtol=5e-2, atol=atol)


def test_captured_loop_equals_eager(model):
    ids = _ids(2, 9)
    assert torch.equal(model.generate_graphed(ids, 6),
                       model.generate(ids, max_new_tokens=6))
