"""CPU-checkable properties of the MFMA skinny GEMM's host logic."""
import pytest
import torch

from alpa_amd.ops import (_SKINNY_MFMA_LDS, _skinny_mfma_legal_splits,
                          _skinny_mfma_mt, _skinny_mfma_splits, skinny_ok)


@pytest.mark.parametrize("N,K", [(5120, 5120), (15360, 5120), (20480, 5120),
                                 (5120, 20480), (7168, 7168), (9216, 9216),
                                 (128, 512), (192, 768)])
@pytest.mark.parametrize("M", [9, 16, 33, 64])
def test_splits_legal(N, K, M):
    s = _skinny_mfma_splits(N, K, M)
    MT = _skinny_mfma_mt(M)
    assert MT in (16, 32, 64) and MT >= M
    assert s in _skinny_mfma_legal_splits(K, MT)
    assert (K // 256) % s == 0                       # whole pipeline rounds
    assert MT * (K // s + 16) * 2 <= _SKINNY_MFMA_LDS  # the staged x slice


@pytest.mark.parametrize("N,K,M", [(96, 512, 16), (128, 320, 16),
                                   (128, 512, 8), (128, 512, 65)])
def test_outside_the_envelope(N, K, M):
    assert _skinny_mfma_splits(N, K, M) is None


def test_gate_stays_closed_on_cpu():
    from alpa_amd.global_env import global_config
    old = global_config.skinny_gemm
    global_config.skinny_gemm = "1"
    try:
        with torch.no_grad():
            assert not skinny_ok(torch.randn(16, 1, 512).bfloat16(),
                                 torch.randn(640, 512).bfloat16(),
                                 torch.nn.Module())
    finally:
        global_config.skinny_gemm = old
