"""The binding layer refuses a bad operand before it allocates or launches.

Every call here must raise from a check in csrc/bindings.cpp, naming the
operand, and never reach a launcher ("HIP error" is what a launcher's or
the runtime's refusal looks like).  Every case is built so that it would
stay inside its buffers even if the kernel ran: a mismatched operand is the
larger one, a wrong dtype is at least as wide or views a buffer that is, a
strided operand views a larger buffer, and a CPU tensor stands only where
the first thing the binding does with it is the device check.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
EPS = 1e-5


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _z(*shape, dtype=BF16, device="cuda"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _refused(name, fn, *args):
    """fn(*args) is refused by a binding check whose message names `name`."""
    with pytest.raises(RuntimeError,
                       match=rf"(^|\W){re.escape(name)}(\W|$)") as info:
        fn(*args)
    assert "HIP error" not in str(info.value)


# ------------------------------------------------------------------ attention

B, H, S, D = 1, 2, 16, 64


def _bhsd(b=B, h=H, s=S, d=D, dtype=BF16):
    return _z(b, h, s, d, dtype=dtype)


def _strided_d():
    """[B, H, S, D] with stride(3) == 2, over a buffer twice as wide."""
    t = _bhsd(d=2 * D)[..., ::2]
    assert t.shape == (B, H, S, D) and t.stride(3) == 2
    return t


def _fwd_args(**over):
    a = dict(q=_bhsd(), k=_bhsd(), v=_bhsd(), o=_bhsd(),
             lse=_z(B, H, S, dtype=F32), alibi=None, kv_lens=None)
    a.update(over)
    return (a["q"], a["k"], a["v"], a["o"], a["lse"], False, 0.125,
            a["alibi"], a["kv_lens"])


def _wide(d, **over):
    """Every 4-D operand at head_dim d."""
    return dict(q=_bhsd(d=d), k=_bhsd(d=d), v=_bhsd(d=d), o=_bhsd(d=d),
                **over)


ATTN_FWD_CASES = {
    # k: batch, heads, head_dim (its length is free: S != Skv is legal)
    "k_batch": ("k", lambda: dict(k=_bhsd(b=B + 1))),
    "k_heads": ("k", lambda: dict(k=_bhsd(h=H + 1))),
    "k_head_dim": ("k", lambda: dict(k=_bhsd(d=D + 16))),
    "v_batch": ("v", lambda: dict(v=_bhsd(b=B + 1))),
    "v_heads": ("v", lambda: dict(v=_bhsd(h=H + 1))),
    "v_len": ("v", lambda: dict(v=_bhsd(s=S + 16))),
    "v_head_dim": ("v", lambda: dict(v=_bhsd(d=D + 16))),
    "o_batch": ("o", lambda: dict(o=_bhsd(b=B + 1))),
    "o_heads": ("o", lambda: dict(o=_bhsd(h=H + 1))),
    "o_len": ("o", lambda: dict(o=_bhsd(s=S + 16))),
    "o_head_dim": ("o", lambda: dict(o=_bhsd(d=D + 16))),
    "q_fp32": ("q", lambda: dict(q=_bhsd(dtype=F32))),
    "k_3d": ("k", lambda: dict(k=_z(H, S, D))),
    "q_strided": ("q", lambda: dict(q=_strided_d())),
    "k_strided": ("k", lambda: dict(k=_strided_d())),
    "v_strided": ("v", lambda: dict(v=_strided_d())),
    "o_strided": ("o", lambda: dict(o=_strided_d())),
    "lse_fp64": ("lse", lambda: dict(lse=_z(B, H, S, dtype=torch.float64))),
    "lse_long": ("lse", lambda: dict(lse=_z(B, H, S + 1, dtype=F32))),
    "alibi_fp64": ("alibi", lambda: dict(alibi=_z(H, dtype=torch.float64))),
    "alibi_long": ("alibi", lambda: dict(alibi=_z(H + 1, dtype=F32))),
    "alibi_cpu": ("alibi", lambda: dict(alibi=_z(H, dtype=F32,
                                                 device="cpu"))),
    "kv_lens_int64": ("kv_lens",
                      lambda: dict(kv_lens=_z(B, dtype=torch.int64))),
    "kv_lens_long": ("kv_lens",
                     lambda: dict(kv_lens=_z(B + 1, dtype=torch.int32))),
    "kv_lens_cpu": ("kv_lens", lambda: dict(
        kv_lens=_z(B, dtype=torch.int32, device="cpu"))),
    "head_dim_72": ("head_dim", lambda: _wide(72)),
    "head_dim_256_alibi": ("alibi",
                           lambda: _wide(256, alibi=_z(H, dtype=F32))),
    "head_dim_256_kv_lens": ("kv_lens", lambda: _wide(
        256, kv_lens=_z(B, dtype=torch.int32))),
}


@pytest.mark.parametrize("case", sorted(ATTN_FWD_CASES))
def test_attn_fwd_out_refuses(ext, case):
    name, over = ATTN_FWD_CASES[case]
    _refused(name, ext.attn_fwd_out, *_fwd_args(**over()))


# the allocating form takes the same inputs minus o and lse
@pytest.mark.parametrize("case", sorted(
    c for c in ATTN_FWD_CASES if ATTN_FWD_CASES[c][0] not in ("o", "lse")))
def test_attn_fwd_refuses(ext, case):
    name, over = ATTN_FWD_CASES[case]
    q, k, v, _, _, causal, scale, alibi, kv_lens = _fwd_args(**over())
    _refused(name, ext.attn_fwd, q, k, v, causal, scale, alibi, kv_lens)


_BWD_4D = ("dout", "q", "k", "v", "o", "dq", "dk", "dv")


def _bwd_args(**over):
    a = {n: _bhsd() for n in _BWD_4D}
    a.update(lse=_z(B, H, S, dtype=F32), alibi=None)
    a.update(over)
    return (a["dout"], a["q"], a["k"], a["v"], a["o"], a["lse"], a["dq"],
            a["dk"], a["dv"], True, 0.125, a["alibi"])


ATTN_BWD_CASES = {
    # a longer k alone is legal (then v is the one that disagrees)
    "k_size": ("k", lambda: dict(k=_bhsd(b=B + 1))),
    "lse_long": ("lse", lambda: dict(lse=_z(B, H, S + 1, dtype=F32))),
    "lse_fp64": ("lse", lambda: dict(lse=_z(B, H, S, dtype=torch.float64))),
    "head_dim_256": ("head_dim", lambda: {n: _bhsd(d=256) for n in _BWD_4D}),
    "alibi_cpu": ("alibi", lambda: dict(alibi=_z(H, dtype=F32,
                                                 device="cpu"))),
}
for _n in ("v", "o", "dout", "dq", "dk", "dv"):
    ATTN_BWD_CASES[f"{_n}_size"] = (
        _n, lambda _n=_n: {_n: _bhsd(s=S + 16)})
for _n in ("k", "v", "o", "dout", "dq", "dk", "dv"):
    ATTN_BWD_CASES[f"{_n}_fp32"] = (
        _n, lambda _n=_n: {_n: _bhsd(dtype=F32)})


@pytest.mark.parametrize("case", sorted(ATTN_BWD_CASES))
def test_attn_bwd_out_refuses(ext, case):
    name, over = ATTN_BWD_CASES[case]
    _refused(name, ext.attn_bwd_out, *_bwd_args(**over()))


@pytest.mark.parametrize("case", sorted(
    c for c in ATTN_BWD_CASES
    if ATTN_BWD_CASES[c][0] not in ("dq", "dk", "dv")))
def test_attn_bwd_refuses(ext, case):
    name, over = ATTN_BWD_CASES[case]
    dout, q, k, v, o, lse, _, _, _, causal, scale, alibi = \
        _bwd_args(**over())
    _refused(name, ext.attn_bwd, dout, q, k, v, o, lse, causal, scale,
             alibi)


# -------------------------------------------------------------- cross entropy

N, V = 4, 64


def _ce_args(**over):
    a = dict(dloss=_z(N, dtype=F32), logits=_z(N, V),
             targets=_z(N, dtype=torch.int64), lse=_z(N, dtype=F32))
    a.update(over)
    return a


CE_CASES = {
    # 4 int32 in front of a buffer that holds 4 int64
    "targets_int32": ("targets", lambda: dict(
        targets=_z(2 * N, dtype=torch.int32)[:N])),
    "targets_long": ("targets",
                     lambda: dict(targets=_z(N + 1, dtype=torch.int64))),
    "targets_strided": ("targets", lambda: dict(
        targets=_z(2 * N, dtype=torch.int64)[::2])),
    "targets_cpu": ("targets", lambda: dict(
        targets=_z(N, dtype=torch.int64, device="cpu"))),
    "vocab_12": ("logits", lambda: dict(logits=_z(N, 12))),
    "lse_long": ("lse", lambda: dict(lse=_z(N + 1, dtype=F32))),
    # 4 bf16 in front of a buffer that holds 4 fp32
    "lse_bf16": ("lse", lambda: dict(lse=_z(2 * N)[:N])),
    "dloss_long": ("dloss", lambda: dict(dloss=_z(N + 1, dtype=F32))),
}


@pytest.mark.parametrize("case", sorted(
    c for c in CE_CASES if CE_CASES[c][0] in ("targets", "logits")))
def test_cross_entropy_fwd_refuses(ext, case):
    name, over = CE_CASES[case]
    a = _ce_args(**over())
    _refused(name, ext.cross_entropy_fwd, a["logits"], a["targets"])


@pytest.mark.parametrize("case", sorted(CE_CASES))
def test_cross_entropy_bwd_refuses(ext, case):
    name, over = CE_CASES[case]
    a = _ce_args(**over())
    _refused(name, ext.cross_entropy_bwd, a["dloss"], a["logits"],
             a["targets"], a["lse"])


# ---------------------------------------------------------------- skinny GEMM

GN, GK = 64, 64


def _skinny_args(N=GN, K=GK, splits=1, **over):
    a = dict(wp=_z(K // 8, N, 8), x=_z(1, K), wscale=None, bias=None)
    a.update(over)
    return a["wp"], a["x"], a["wscale"], a["bias"], N, K, splits


SKINNY_CASES = {
    "wp_long": ("wp", lambda: _skinny_args(wp=_z(GN * GK + 8))),
    "wp_fp32": ("wp", lambda: _skinny_args(wp=_z(GK // 8, GN, 8,
                                                 dtype=F32))),
    # an e4m3 scale with bf16 weights: wp must then hold one-byte elements
    "wscale_with_bf16_wp": ("wp", lambda: _skinny_args(
        wscale=torch.ones(1, device="cuda"))),
    "bias_long": ("bias", lambda: _skinny_args(bias=_z(GN + 8))),
    "bias_fp32": ("bias", lambda: _skinny_args(bias=_z(GN, dtype=F32))),
    "N_96": ("N", lambda: _skinny_args(N=96)),
    "K_96": ("K", lambda: _skinny_args(K=96)),
    "splits_0": ("splits", lambda: _skinny_args(splits=0)),
    "splits_3_of_2": ("splits", lambda: _skinny_args(K=128, splits=3)),
    "x_fp32": ("x", lambda: _skinny_args(x=_z(1, GK, dtype=F32))),
}


@pytest.mark.parametrize("case", sorted(SKINNY_CASES))
def test_skinny_gemm_refuses(ext, case):
    name, args = SKINNY_CASES[case]
    _refused(name, ext.skinny_gemm, *args())


# -------------------------------------------------------------------- width 0

def _w0():
    return _z(N, 0)


def _st():
    return _z(N, dtype=F32)


WIDTH0_CALLS = {
    "layer_norm_fwd": ("x", lambda e: e.layer_norm_fwd(_w0(), _z(0), _z(0),
                                                       EPS)),
    "layer_norm_bwd": ("x", lambda e: e.layer_norm_bwd(_w0(), _w0(), _z(0),
                                                       _st(), _st())),
    "add_layer_norm_fwd": ("a", lambda e: e.add_layer_norm_fwd(
        _w0(), None, _z(0), _z(0), EPS)),
    "add_layer_norm_bwd": ("h", lambda e: e.add_layer_norm_bwd(
        _w0(), None, _w0(), _z(0), _st(), _st())),
    "bias_gelu_fwd": ("x", lambda e: e.bias_gelu_fwd(_w0(), _z(0))),
    "bias_gelu_bwd": ("x", lambda e: e.bias_gelu_bwd(_w0(), _w0(), _z(0))),
    "colsum_bf16": ("t", lambda e: e.colsum_bf16(_w0())),
    "cross_entropy_fwd": ("logits", lambda e: e.cross_entropy_fwd(
        _w0(), _z(N, dtype=torch.int64))),
    "cross_entropy_bwd": ("logits", lambda e: e.cross_entropy_bwd(
        _st(), _w0(), _z(N, dtype=torch.int64), _st())),
}


@pytest.mark.parametrize("entry", sorted(WIDTH0_CALLS))
def test_width_zero_is_refused(ext, entry):
    """A [4, 0] tensor is refused by the rows check, which sits right
    before the only division of numel() by a width."""
    name, call = WIDTH0_CALLS[entry]
    _refused(name, call, ext)


# --------------------------------------------------------------- AdamW tables
# All-zero tables: one chunk of a tensor of 0 elements.

def _tables(**over):
    a = dict(descs=_z(1, 6, dtype=torch.int64),
             chunks=_z(1, 2, dtype=torch.int32))
    a.update(over)
    return a["descs"], a["chunks"]


TABLE_CASES = {
    # 6 int32 in front of a buffer that holds 6 int64
    "descs_int32": ("descs", lambda: dict(
        descs=_z(12, dtype=torch.int32)[:6].view(1, 6))),
    # [1, 5] in front of a buffer that holds [1, 6]
    "descs_5_cols": ("descs", lambda: dict(
        descs=_z(6, dtype=torch.int64)[:5].view(1, 5))),
    "chunks_int64": ("chunks", lambda: dict(
        chunks=_z(1, 2, dtype=torch.int64))),
    "chunks_3_cols": ("chunks", lambda: dict(
        chunks=_z(1, 3, dtype=torch.int32))),
}


@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_adamw_tables_refused(ext, case):
    name, over = TABLE_CASES[case]
    descs, chunks = _tables(**over())
    _refused(name, ext.adamw_step_raw, descs, chunks, 1, 1e-3, 0.9, 0.95,
             1e-8, 0.0, 1.0)
    _refused(name, ext.multi_tensor_sumsq_raw, descs, chunks,
             _z(1, dtype=F32), _z(1, dtype=F32))


# --------------------------------------------------------------------- probes

@pytest.mark.parametrize("entry,m,k", [("mfma_probe", 16, 32),
                                       ("mfma_probe32", 32, 16)])
def test_mfma_probes_refuse_fp32_b(ext, entry, m, k):
    _refused("b", getattr(ext, entry), _z(m, k), _z(k, m, dtype=F32))


# -------------------------------------------------------------- mixed devices

def test_operands_on_two_devices_are_refused(ext):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    x = _z(N, 64, device="cuda:0")
    _refused("w", ext.layer_norm_fwd, x, _z(64, device="cuda:1"),
             _z(64, device="cuda:0"), EPS)
