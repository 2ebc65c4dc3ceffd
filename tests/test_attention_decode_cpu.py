"""The decode-attention case builders check themselves, and
ops.flash_attention_decode on the CPU (the reference path) agrees with
them: what test_attention_decode_gpu.py then asks of the kernel is right.

Chunk-relative lengths are built from ops.DECODE_ATTN_CHUNK, as on the GPU.
"""
import math

import pytest
import torch

import attn_decode_cases as DC
import attn_fwd_cases as F
from alpa_amd import ops


def _shape(D, Skv, kv_lens):
    return DC.resolve(ops.DECODE_ATTN_CHUNK(D), Skv, kv_lens)


def _decode(case):
    return ops.flash_attention_decode(case.q, case.k, case.v, case.kv_lens,
                                      case.scale, case.alibi)


def _check_fp64(o, case):
    o64, _, A = F.reference_fp64(case)
    ratio = F.bound_ratio(o, o64, A)
    print(f"err/bound {ratio:.3f}")
    assert ratio <= 1.0


def test_chunk_is_a_function_of_head_dim():
    for D in DC.HEAD_DIMS:
        assert ops.DECODE_ATTN_CHUNK(D) in (128, 256, 512)
    with pytest.raises(ValueError):
        ops.DECODE_ATTN_CHUNK(272)


def test_exact_shapes_cover_the_edges():
    """Every head dim and every Skv of the list, an empty slot next to a
    full one, and every length of {0, 1, C-1, C, C+1, Skv}."""
    assert {s[0] for s in DC.EXACT_SHAPES} == set(DC.HEAD_DIMS)
    assert {s[1] for s in DC.EXACT_SHAPES} == {"1", "C-1", "C", "C+1",
                                               "2C+1"}
    pairs = [s[2] for s in DC.EXACT_SHAPES if s[2] is not None]
    assert {x for p in pairs for x in p} == {"0", "1", "C-1", "C", "C+1",
                                             "S"}
    assert ("0", "S") in pairs or ("S", "0") in pairs


@pytest.mark.parametrize("D,Skv,kv_lens", DC.EXACT_SHAPES)
def test_one_hot(D, Skv, kv_lens):
    n, lens = _shape(D, Skv, kv_lens)
    case = DC.one_hot(n, D, lens)
    assert case.info["min_gap"] >= 128.0
    o = _decode(case)
    assert o.shape == (F.B, F.H, 1, D) and o.dtype == torch.bfloat16
    assert torch.equal(o, case.o)
    _, lse64, _ = F.reference_fp64(case)
    assert torch.equal(lse64.to(torch.float32), case.lse)


@pytest.mark.parametrize("D,Skv,kv_lens", DC.EXACT_SHAPES)
def test_uniform(D, Skv, kv_lens):
    """The builder has asserted that fp32 sum * (1/n) and sum / n both round
    to the expected bf16; the expectation is the fp64 one."""
    n, lens = _shape(D, Skv, kv_lens)
    case = DC.uniform(n, D, lens)
    o64, lse64, _ = F.reference_fp64(case)
    assert torch.equal(o64.to(torch.bfloat16), case.o)
    some = case.info["n"] > 0
    assert bool((lse64[some] == case.info["lse64"][some]).all())
    assert bool((case.lse[~some] == -math.inf).all())
    _check_fp64(_decode(case), case)


@pytest.mark.parametrize("D,alibi,kv_lens", DC.RANDOM_SHAPES)
def test_random(D, alibi, kv_lens):
    n, lens = _shape(D, "2C+1", kv_lens)
    _check_fp64(_decode(DC.random_case(n, D, alibi, lens)), DC.random_case(
        n, D, alibi, lens))


@pytest.mark.parametrize("D,order", DC.STAIR_SHAPES)
def test_staircase(D, order):
    n, _ = _shape(D, "2C+1", None)
    case = DC.staircase(n, D, order)
    _check_fp64(_decode(case), case)


def test_decode_matches_flash_attention_on_cpu():
    """Off the GPU both names are the reference: same bits, and kv_lens of
    the full length changes nothing."""
    case = DC.random_case(70, 64, False, None)
    o = _decode(case)
    assert torch.equal(o, ops.flash_attention(case.q, case.k, case.v,
                                              causal=False))
    full = torch.full((F.B,), 70, dtype=torch.int32)
    assert torch.equal(o, ops.flash_attention_decode(case.q, case.k, case.v,
                                                     full))
    assert not ops.decode_attn_ok(case.q, case.k, case.v)
