"""MXFP4 format on the CPU: the quantizer's bytes on hand-checked blocks, the
exact round trip, and the reference linear."""
import pytest
import torch

import mxfp4_cases as MC
from alpa_amd import ops
from alpa_amd.ops import reference as ref


def test_hand_checked_bytes():
    w, scales, codes = MC.rows()
    got_codes, got_scales = ops.mxfp4_quantize(w)
    for i, case in enumerate(MC.CASES):
        assert got_scales[i].tolist() == scales[i].tolist(), case[0]
        assert got_codes[i].tolist() == codes[i].tolist(), case[0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_round_trip_is_exact(dtype):
    """Every code under scale bytes from one clamp to the other, in the
    low and in the high nibble; 4 rows x 8 blocks."""
    codes, _ = MC.all_codes(4, 256)
    scales = torch.tensor([2, 3, 100, 126, 127, 128, 200, 252],
                          dtype=torch.uint8).repeat(4, 1)
    w = ops.mxfp4_dequantize(codes, scales, dtype)
    assert w.dtype == dtype and torch.isfinite(w).all()
    assert len(w[0, :32].float().unique()) == 15  # +0 and -0 are one value
    c2, s2 = ops.mxfp4_quantize(w)
    assert torch.equal(s2, scales)
    assert torch.equal(ops.mxfp4_dequantize(c2, s2, dtype), w)
    # the only codes that may differ are the two zeros' signs kept apart
    assert torch.equal(c2 & 0x77, codes & 0x77)


def test_reference_linear_is_fp32_on_the_dequantized_weights():
    codes, scales = MC.all_codes(64, 256)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (3, 256), generator=g).to(torch.bfloat16)
    b = torch.randint(-2, 3, (64,), generator=g).to(torch.bfloat16)
    w = ops.mxfp4_dequantize(codes, scales)
    want = (x.double() @ w.double().t() + b.double()).to(torch.bfloat16)
    assert torch.equal(ref.skinny_linear_fp4(x, codes, scales, b), want)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_weight_raises(bad):
    w = torch.ones(2, 64)
    w[1, 40] = bad
    with pytest.raises(ValueError):
        ops.mxfp4_quantize(w)
