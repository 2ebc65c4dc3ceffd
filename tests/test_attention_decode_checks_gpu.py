"""The attn_decode binding refuses a bad operand before it allocates or
launches: one case per check, in the manner of test_binding_checks_gpu.py.

Every call must raise from a check in csrc/bindings.cpp, naming the operand,
and never reach the launcher ("HIP error" is what a launcher's or the
runtime's refusal looks like).  Every case would stay inside its buffers
even if the kernel ran: a mismatched operand is the larger one, a strided
operand views a larger buffer."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
B, H, SKV, D = 2, 2, 16, 64


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _z(*shape, dtype=BF16, device="cuda"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _args(d=D, **over):
    a = dict(q=_z(B, H, 1, d), k=_z(B, H, SKV, d), v=_z(B, H, SKV, d),
             alibi=None, kv_lens=None)
    a.update(over)
    return a["q"], a["k"], a["v"], 0.125, a["alibi"], a["kv_lens"]


def _odd_row_stride():
    """[B, H, SKV, D] whose rows are D + 4 elements apart: 8 bytes off a
    16-byte boundary on every second row."""
    t = _z(B, H, SKV, D + 4)[..., :D]
    assert t.stride(2) == D + 4 and t.stride(3) == 1
    return t


def _odd_base():
    """[B, H, SKV, D] that starts 4 elements into its buffer."""
    t = _z(B * H * SKV * D + 8)[4:4 + B * H * SKV * D].view(B, H, SKV, D)
    assert t.data_ptr() % 16 == 8
    return t


CASES = {
    "q_fp32": ("q", lambda: _args(q=_z(B, H, 1, D, dtype=F32))),
    "k_fp32": ("k", lambda: _args(k=_z(B, H, SKV, D, dtype=F32))),
    "q_two_rows": ("q", lambda: _args(q=_z(B, H, 2, D))),
    "q_3d": ("q", lambda: _args(q=_z(H, 1, D))),
    "head_dim_24": ("head_dim", lambda: _args(d=24)),
    "head_dim_272": ("head_dim", lambda: _args(d=272)),
    "k_heads": ("k", lambda: _args(k=_z(B, H + 1, SKV, D))),
    "k_head_dim": ("k", lambda: _args(k=_z(B, H, SKV, D + 16))),
    "v_len": ("v", lambda: _args(v=_z(B, H, SKV + 16, D))),
    "v_batch": ("v", lambda: _args(v=_z(B + 1, H, SKV, D))),
    "kv_lens_int64": ("kv_lens",
                      lambda: _args(kv_lens=_z(B, dtype=torch.int64))),
    "kv_lens_long": ("kv_lens",
                     lambda: _args(kv_lens=_z(B + 1, dtype=torch.int32))),
    "kv_lens_cpu": ("kv_lens", lambda: _args(
        kv_lens=_z(B, dtype=torch.int32, device="cpu"))),
    "alibi_long": ("alibi", lambda: _args(alibi=_z(H + 1, dtype=F32))),
    "alibi_fp64": ("alibi", lambda: _args(alibi=_z(H,
                                                   dtype=torch.float64))),
    "k_row_stride": ("k", lambda: _args(k=_odd_row_stride())),
    "v_row_stride": ("v", lambda: _args(v=_odd_row_stride())),
    "k_base": ("k", lambda: _args(k=_odd_base())),
    "k_strided_d": ("k", lambda: _args(k=_z(B, H, SKV, 2 * D)[..., ::2])),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_attn_decode_refuses(ext, case):
    name, args = CASES[case]
    with pytest.raises(RuntimeError,
                       match=rf"(^|\W){re.escape(name)}(\W|$)") as info:
        ext.attn_decode(*args())
    assert "HIP error" not in str(info.value)


@pytest.mark.parametrize("case", ["k_row_stride", "k_base", "q_two_rows",
                                  "head_dim_24", "q_fp32"])
def test_envelope_predicate_agrees(case):
    """ops.decode_attn_ok is false where the binding refuses the views."""
    from alpa_amd import ops
    q, k, v = CASES[case][1]()[:3]
    assert not ops.decode_attn_ok(q, k, v)
    q, k, v = _args()[:3]
    assert ops.decode_attn_ok(q, k, v)
