"""forward_step over a prompt in pieces (chunked prefill: every piece after
the first attends to the cache causally at its end) against one forward_step
over the whole prompt, for the three decoder families on the fp32 CPU path,
with the bf16-free cache and with the reference e4m3 cache."""
import pytest
import torch

from alpa_amd.global_env import global_config
from alpa_amd.models.bloom import BloomConfig, BloomModel
from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
from alpa_amd.models.opt import OPTConfig, OPTModel

CFG = dict(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
           max_seq_len=64)
PIECES = (5, 4, 1)


def build(name):
    if name == "opt":
        return OPTModel(OPTConfig(**CFG), None, 1, torch.float32, None,
                        init_seed=13)
    if name == "bloom":
        return BloomModel(BloomConfig(**CFG), init_seed=19)
    return CodeGenModel(CodeGenConfig(rotary_dim=8, **CFG), init_seed=17)


def prompt():
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, CFG["vocab_size"], (2, sum(PIECES)), generator=g)


@pytest.mark.parametrize("name", ["opt", "bloom", "codegen"])
@torch.no_grad()
def test_prompt_in_pieces_matches_one_pass(name):
    m, ids = build(name), prompt()
    whole = m.forward_step(ids, m.new_cache(2))
    cache, at = m.new_cache(2), 0
    for n in PIECES:
        logits = m.forward_step(ids[:, at:at + n], cache)
        at += n
    assert cache.length == ids.shape[1]
    torch.testing.assert_close(logits, whole, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("name", ["opt", "bloom", "codegen"])
@torch.no_grad()
def test_pieces_over_the_e4m3_cache_match_single_tokens(monkeypatch, name):
    """With the e4m3 cache a piece reads quantized history, as single-token
    steps do: 5 tokens, then 4 + 1 as pieces, against 5 tokens, then five
    single-token steps."""
    monkeypatch.setattr(global_config, "kv_cache_fp8", True)
    m, ids = build(name), prompt()
    first = PIECES[0]
    cache = m.new_cache(2)
    assert cache.fp8
    m.forward_step(ids[:, :first], cache)
    for t in range(first, ids.shape[1]):
        single = m.forward_step(ids[:, t:t + 1], cache)
    cache, at = m.new_cache(2), 0
    for n in PIECES:
        logits = m.forward_step(ids[:, at:at + n], cache)
        at += n
    torch.testing.assert_close(logits, single, rtol=2e-4, atol=2e-4)
