"""The cases of test_attention_fwd_d80_gpu.py, checked without a GPU the way
test_attention_fwd_cases_cpu.py checks the older shapes: every builder's own
assertions run, and both the fp32 CPU reference and the emulation of the
kernel's tile loop meet the expectations the kernel is held to, at the same
bounds."""
import math

import pytest
import torch

import attn_fwd_cases as C
import attn_fwd_d80_shapes as SH
from alpa_amd.ops import reference as ref


def _ref(case):
    return ref.attention_fwd(case.q.float(), case.k.float(), case.v.float(),
                             case.causal, case.scale, case.alibi,
                             case.kv_lens)


def _check_uniform_lse(lse, case):
    n = case.info["n"]
    some = n > 0
    assert bool((lse[~some] == -math.inf).all())
    err = (lse.double() - case.info["lse64"])[some].abs()
    assert float(err.max() if err.numel() else 0.0) <= 1e-4


def _check_fp64(o, lse, case):
    o64, lse64, A = C.reference_fp64(case)
    assert C.bound_ratio(o, o64, A) <= 1.0
    torch.testing.assert_close(lse.double(), lse64, rtol=0, atol=C.LSE_ATOL)


def test_shape_lists():
    """The builders' limits, and what the shapes are there to reach."""
    views = [(S, S, d, causal) for S, d, causal in SH.VIEW_SHAPES]
    for s in SH.AB_SHAPES + views:
        assert s[1] <= 256                      # distinct 8-bit codes
    for group in (SH.AB_SHAPES, SH.STAIR_SHAPES, SH.RANDOM_SHAPES,
                  [SH.TAIL_SHAPE]):
        assert all(s[0] <= 320 and s[1] <= 320 for s in group)
    # two q blocks whose second sees interior, diagonal and skipped tiles
    assert (256, 256, 80, True) in SH.AB_SHAPES
    assert any(c and skv > s for s, skv, _, c in SH.AB_SHAPES)
    assert any(c and skv < s for s, skv, _, c in SH.AB_SHAPES)
    S, Skv, D, lens = SH.TAIL_SHAPE
    assert D == 80 and all(0 < n < Skv for n in lens)
    assert any(n % C.TILE for n in lens) and any(n % C.TILE == 0 for n in lens)


@pytest.mark.parametrize(
    "shape", SH.AB_SHAPES + [(S, S, d, c) for S, d, c in SH.VIEW_SHAPES])
def test_one_hot(shape):
    case = C.one_hot(*shape)   # asserts the gap of 128
    assert case.info["min_gap"] >= 128.0
    for o, lse in (_ref(case)[:2], C.emulate(case)[:2]):
        assert torch.equal(o.to(torch.bfloat16), case.o)
        assert torch.equal(lse, case.lse)


def test_one_hot_matches_in_every_tile():
    """Keys are matched in all four kv tiles, so rows meet their key both on
    the deferred path and after a rescale with alpha = 0."""
    case = C.one_hot(256, 256, 80, True)
    assert case.info["matched_tiles"] == [0, 1, 2, 3]
    assert C.emulate(case)[2]["late_rescales"] > 0


@pytest.mark.parametrize("shape", SH.AB_SHAPES)
def test_uniform(shape):
    case = C.uniform(*shape)
    o, lse, _ = C.emulate(case)
    assert torch.equal(o, case.o)
    _check_uniform_lse(lse, case)
    o, lse = _ref(case)
    o64, _, A = C.reference_fp64(case)
    assert C.bound_ratio(case.o, o64, A) <= 1.0
    assert C.bound_ratio(o, o64, A) <= 1.0
    _check_uniform_lse(lse, case)


def test_poison_tail_changes_only_the_tail():
    S, Skv, D, lens = SH.TAIL_SHAPE
    case = C.uniform(S, Skv, D, False, kv_lens=lens)
    bad = C.poison_tail(C.poison_tail(case, "k", math.nan), "v", math.nan)
    for b, n in enumerate(lens):
        for clean, dirty in ((case.k, bad.k), (case.v, bad.v)):
            assert torch.equal(clean[b, :, :n], dirty[b, :, :n])
            assert bool(torch.isnan(dirty[b, :, n:]).all())
    # the emulation, like the kernel, never observes the tail
    o, lse, _ = C.emulate(bad)
    assert torch.equal(o, case.o)
    _check_uniform_lse(lse, case)


@pytest.mark.parametrize("shape", SH.STAIR_SHAPES)
def test_staircase(shape):
    case = C.staircase(*shape)   # asserts that the staircase is bf16-exact
    o, lse, stats = C.emulate(case)
    _check_fp64(o, lse, case)
    _check_fp64(*_ref(case)[:2], case)
    a = stats["alphas"]
    if shape[4] == "asc":
        assert stats["late_rescales"] >= 10
        assert int(((a > 1e-3) & (a < 1.0)).sum()) >= 10
    elif shape[4] == "desc":
        assert stats["late_rescales"] == 0


@pytest.mark.parametrize("shape", SH.RANDOM_SHAPES)
def test_random(shape):
    case = C.random_case(*shape)
    o, lse, _ = C.emulate(case)
    _check_fp64(o, lse, case)
    _check_fp64(*_ref(case)[:2], case)
