"""reference.qkv_cache_write, the specification of csrc/qkv_cache_write.hip,
against the torch ops it stands for: apply_rotary, kv_cache_append_fp8 and a
plain copy."""
import pytest
import torch

from alpa_amd.models.codegen import apply_rotary, rotary_tables
from alpa_amd.ops import reference as ref

B, S, H, D, L, RD, POS = 2, 3, 2, 16, 8, 8, 2


def _inputs():
    qkv = torch.randn(B, S, H, 3, D, generator=torch.Generator().manual_seed(1))
    q, k, v = (qkv[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))
    return qkv, q, k, v


@pytest.mark.parametrize("fp8", [False, True])
def test_rotary_is_apply_rotary(fp8):
    """fp32 inputs and tables: q and k equal apply_rotary exactly; the e4m3
    rows equal kv_cache_append_fp8 of the rotated k and of v."""
    qkv, q, k, v = _inputs()
    sin, cos = rotary_tables(RD, 16, torch.float32, "cpu")
    want_q, want_k = (apply_rotary(t, sin, cos, POS, RD) for t in (q, k))

    def cache():
        if not fp8:
            return torch.full((B, H, L, D), 7.0), torch.full((B, H, L, D), 7.0)
        return tuple((torch.zeros(B, H, L, D).to(torch.float8_e4m3fn),
                      torch.full((B, H, L), 7.0)) for _ in range(2))

    ck, cv = cache()
    got_q, got_k = ref.qkv_cache_write(qkv, ck, cv, POS, (sin, cos, RD),
                                       want_k=True)
    assert got_q.is_contiguous() and torch.equal(got_q, want_q)
    assert torch.equal(got_k, want_k)
    if not fp8:
        assert torch.equal(ck[:, :, POS:POS + S], want_k)
        assert torch.equal(cv[:, :, POS:POS + S], v)
        assert bool((ck[:, :, :POS] == 7).all() and (cv[:, :, POS + S:] == 7).all())
        return
    (wk, wks), (wv, wvs) = cache()
    ref.kv_cache_append_fp8(want_k, v, wk, wks, wv, wvs, POS)
    for got, want in ((ck[0], wk), (ck[1], wks), (cv[0], wv), (cv[1], wvs)):
        assert torch.equal(got.float(), want.float())


def test_no_rotary_is_a_copy_and_bad_rows_are_masked():
    """rotary=None copies; slot 1 starts at L - 1, so its rows 1 and 2 are
    zero in q and touch nothing."""
    qkv, q, k, v = _inputs()
    ck, cv = torch.full((B, H, L, D), 7.0), torch.full((B, H, L, D), 7.0)
    got = ref.qkv_cache_write(qkv, ck, cv, torch.tensor([0, L - 1]))
    assert torch.equal(got[0], q[0]) and torch.equal(got[1, :, :1], q[1, :, :1])
    assert bool((got[1, :, 1:] == 0).all())
    assert torch.equal(ck[0, :, :S], k[0]) and torch.equal(cv[0, :, :S], v[0])
    assert torch.equal(ck[1, :, L - 1], k[1, :, 0])
    assert bool((ck[0, :, S:] == 7).all() and (ck[1, :, :L - 1] == 7).all())
    sin, cos = rotary_tables(RD, 4, torch.float32, "cpu")
    with pytest.raises(ValueError, match="outside the rotary tables"):
        ref.qkv_cache_write(qkv, ck, cv, 2, (sin, cos, RD))
