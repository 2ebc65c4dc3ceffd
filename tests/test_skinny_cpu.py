"""CPU-checkable properties of the skinny decode GEMV host logic."""
import pytest
import torch

from alpa_amd.ops import _skinny_splits, skinny_ok


@pytest.mark.parametrize("N,K", [(5120, 5120), (15360, 5120),
                                 (20480, 5120), (5120, 20480),
                                 (27648, 9216), (9216, 36864),
                                 (640, 512), (1280, 1024)])
@pytest.mark.parametrize("M", [1, 4, 8])
def test_splits_legal(N, K, M):
    s = _skinny_splits(N, K, M)
    assert s is not None
    rounds = K // 8 // s
    MT = 4
    while MT < M:
        MT *= 2
    assert (K // 8) % s == 0          # launcher divisibility
    assert rounds % 8 == 0            # kernel's 8-deep pipeline
    assert rounds * 16 * MT <= 65536  # LDS x-slice fits 64 KB


def test_gate_is_inference_only_and_shape_gated():
    from alpa_amd.global_env import global_config
    w = torch.randn(5120, 5120)
    x = torch.randn(4, 1, 5120)

    class M(torch.nn.Module):
        pass
    m = M()
    # CPU tensors never take the HIP path
    with torch.no_grad():
        assert not skinny_ok(x, w, m)
    # the envelope check itself (device-independent part): big square
    # bf16 shapes are excluded in auto mode unless fp8-packed
    old = global_config.fp8_gemm
    global_config.fp8_gemm = False
    try:
        wbig = torch.randn(9216, 9216)
        with torch.no_grad():
            assert not skinny_ok(torch.randn(4, 1, 9216), wbig, m)
    finally:
        global_config.fp8_gemm = old



# _skinny_splits(N, K, M) for N, K in _SKINNY_DIMS and M in _SKINNY_MS, as the
# function stood before the padded-M tier and the legal-split list became
# _skinny_mt and _skinny_legal_splits.  One row per (N, K), one entry per M.
# Every shape of this grid has a legal split (s = K/64 leaves 8 rounds, 8 KB
# of LDS at MT = 64), so no entry is None.
_SKINNY_DIMS = (64, 2560, 5120, 7168, 20480)
_SKINNY_MS = (1, 4, 5, 8, 64)
_SKINNY_SPLITS = {
    (64, 64): (1, 1, 1, 1, 1),
    (64, 2560): (40, 40, 40, 40, 40),
    (64, 5120): (80, 80, 80, 80, 80),
    (64, 7168): (112, 112, 112, 112, 112),
    (64, 20480): (320, 320, 320, 320, 320),
    (2560, 64): (1, 1, 1, 1, 1),
    (2560, 2560): (40, 40, 40, 40, 40),
    (2560, 5120): (40, 40, 40, 40, 40),
    (2560, 7168): (56, 56, 56, 56, 56),
    (2560, 20480): (160, 160, 160, 160, 160),
    (5120, 64): (1, 1, 1, 1, 1),
    (5120, 2560): (20, 20, 20, 20, 20),
    (5120, 5120): (40, 40, 40, 40, 40),
    (5120, 7168): (56, 56, 56, 56, 56),
    (5120, 20480): (160, 160, 160, 160, 160),
    (7168, 64): (1, 1, 1, 1, 1),
    (7168, 2560): (20, 20, 20, 20, 20),
    (7168, 5120): (40, 40, 40, 40, 40),
    (7168, 7168): (56, 56, 56, 56, 56),
    (7168, 20480): (160, 160, 160, 160, 160),
    (20480, 64): (1, 1, 1, 1, 1),
    (20480, 2560): (20, 20, 20, 20, 20),
    (20480, 5120): (40, 40, 40, 40, 40),
    (20480, 7168): (56, 56, 56, 56, 56),
    (20480, 20480): (160, 160, 160, 160, 160),
}


def test_skinny_splits_literals():
    assert set(_SKINNY_SPLITS) == {(N, K) for N in _SKINNY_DIMS
                                   for K in _SKINNY_DIMS}
    for (N, K), want in _SKINNY_SPLITS.items():
        got = tuple(_skinny_splits(N, K, M) for M in _SKINNY_MS)
        assert got == want, (N, K, got, want)
