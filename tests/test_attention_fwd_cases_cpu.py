"""The input families of test_attention_fwd_exact_gpu.py, checked without a
GPU: every builder's own assertions run for every case the GPU file uses,
and both the fp32 CPU reference and the emulation of the kernel's tile loop
must meet the expectations the kernel is held to, at the same bounds."""
import math

import pytest
import torch

import attn_fwd_cases as C
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


ONE_HOT = [(s, None) for s in C.AB_SHAPES] + \
          [(s[:3] + (False,), s[3]) for s in C.VARLEN_SHAPES]
UNIFORM = [(s, None) for s in C.AB_SHAPES + C.B_ONLY_SHAPES] + \
          [(s[:3] + (False,), s[3])
           for s in C.VARLEN_SHAPES + C.B_ONLY_VARLEN_SHAPES]


def test_case_lists_cover_the_kernel():
    """The shapes the issue names are all present."""
    shapes = C.AB_SHAPES
    assert {s[2] for s in shapes} >= {16, 48, 64, 80, 96, 112, 128, 160, 256}
    assert {s[0] for s in shapes} >= {1, 16, 67, 130, 192, 200}
    assert {s[1] for s in shapes} >= {1, 63, 64, 65, 200, 256}
    assert any(s[1] == 257 for s in C.B_ONLY_SHAPES)
    assert any(c and skv > s for s, skv, _, c in shapes)
    assert any(c and skv < s for s, skv, _, c in shapes)
    lens = {x for s in C.VARLEN_SHAPES for x in s[3]}
    assert lens >= {0, 1, 64, 65}
    assert any(s[1] in s[3] for s in C.VARLEN_SHAPES)
    assert all(s[2] <= 128 and max(s[3]) <= s[1] for s in C.VARLEN_SHAPES)
    for group in (C.AB_SHAPES, C.B_ONLY_SHAPES, C.VARLEN_SHAPES,
                  C.STAIR_SHAPES, C.RANDOM_SHAPES):
        assert all(s[0] <= 320 and s[1] <= 320 for s in group)
    assert set(C.TAIL_SHAPES) <= set(C.VARLEN_SHAPES +
                                     C.B_ONLY_VARLEN_SHAPES)


@pytest.mark.parametrize("shape,lens", ONE_HOT)
def test_one_hot(shape, lens):
    case = C.one_hot(*shape, kv_lens=lens)   # asserts the gap of 128
    assert case.info["min_gap"] >= 128.0
    for o, lse in (_ref(case)[:2], C.emulate(case)[:2]):
        assert torch.equal(o.to(torch.bfloat16), case.o)
        assert torch.equal(lse, case.lse)


def test_one_hot_smallest_gap_and_tiles():
    """D = 16 reaches the gap of exactly 128, and the matched keys lie in
    the first tile (deferred path) and in later ones (alpha = 0)."""
    case = C.one_hot(130, 200, 16, False)
    assert case.info["min_gap"] == 128.0
    assert case.info["matched_tiles"] == [0, 1, 2, 3]
    assert C.emulate(case)[2]["late_rescales"] > 0


def test_one_hot_codes_not_periodic():
    """No shift of the columns by a multiple of 8 maps a key onto itself."""
    k = C.one_hot_codes(256, 64, torch.Generator().manual_seed(0))
    for shift in range(8, 64, 8):
        assert not bool((k == k.roll(shift, -1)).all(-1).any())


@pytest.mark.parametrize("shape,lens", UNIFORM)
def test_uniform(shape, lens):
    """The emulation divides the exact integer sum once, as the kernel does,
    and must be bit-exact.  The reference normalises P to a rounded 1/n
    before the product, so its partial sums k * fl(1/n) round and a zero
    sum comes out as ~1e-9: it is held to the derived bound instead."""
    case = C.uniform(*shape, kv_lens=lens)
    o, lse, _ = C.emulate(case)
    assert torch.equal(o, case.o)
    _check_uniform_lse(lse, case)
    o, lse = _ref(case)
    o64, _, A = C.reference_fp64(case)
    assert C.bound_ratio(case.o, o64, A) <= 1.0
    assert C.bound_ratio(o, o64, A) <= 1.0
    _check_uniform_lse(lse, case)


@pytest.mark.parametrize("shape", C.TAIL_SHAPES)
@pytest.mark.parametrize("which", ["k", "v"])
def test_poison_tail_changes_only_the_tail(shape, which):
    case = C.uniform(*shape[:3], False, kv_lens=shape[3])
    bad = C.poison_tail(case, which, math.nan)
    for b, n in enumerate(shape[3]):
        for clean, dirty in ((case.k, bad.k), (case.v, bad.v)):
            assert torch.equal(clean[b, :, :n], dirty[b, :, :n])
        assert bool(torch.isnan((bad.k if which == "k" else bad.v)
                                [b, :, n:]).all())
    # the emulation, like the kernel, never observes the tail
    o, lse, _ = C.emulate(bad)
    assert torch.equal(o, case.o)


@pytest.mark.parametrize("shape", C.STAIR_SHAPES)
def test_staircase(shape):
    case = C.staircase(*shape)   # asserts that the staircase is bf16-exact
    o, lse, stats = C.emulate(case)
    _check_fp64(o, lse, case)
    _check_fp64(*_ref(case)[:2], case)
    a = stats["alphas"]
    if shape[4] == "asc":
        # the rescale branch is taken after the first tile, and by rows
        # whose alpha lies strictly between 0 and 1
        assert stats["late_rescales"] >= 10
        assert int(((a > 1e-3) & (a < 1.0)).sum()) >= 10
    elif shape[4] == "desc":
        # the maximum is in the first tile: nothing rescales
        assert stats["late_rescales"] == 0


@pytest.mark.parametrize("shape", C.RANDOM_SHAPES)
def test_random(shape):
    case = C.random_case(*shape)
    o, lse, _ = C.emulate(case)
    _check_fp64(o, lse, case)
    _check_fp64(*_ref(case)[:2], case)


def test_randn_never_rescales_late():
    """Why the staircase exists: on randn inputs at 1/sqrt(D) the deferred
    rescale is not taken after the first visible tile."""
    case = C.random_case(130, 200, 112, False, False, None)
    assert C.emulate(case)[2]["late_rescales"] == 0
