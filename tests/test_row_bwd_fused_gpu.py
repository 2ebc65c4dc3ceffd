"""The single-pass backward kernels of bias+GeLU and LayerNorm and the
on-device reduction of their column partials.

layer_norm_bwd / add_layer_norm_bwd run one fused kernel up to H = 4096 and
the dx + dw/db-partial pair above; bias_gelu_bwd writes dx and sums it in
one kernel; every [P, F] partial is reduced by one finalize kernel, straight
into fp32 or bf16.  The oracle is alpa_amd.ops.reference on fp64 copies of
seeded bf16 inputs, and a column sum is held against the exact fp64 sum of
the terms the kernel summed.

Every input is the leading N rows of a buffer whose remaining rows are NaN,
so a row read beyond N shows up in every case as a non-finite output.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import alpa_amd.ops as ops
from alpa_amd.ops import reference as ref

BF16 = torch.bfloat16
F32 = torch.float32
EPS = 1e-5
PAD_ROWS = 4

# stripe counts of the kernels under test (LNF_STRIPES in csrc/layernorm.hip,
# stripes_for in csrc/bindings.cpp)
LN_STRIPES = 1024


def gelu_stripes(N, F):
    return min(max(64, 2048 // max(1, F // 2048)), N, 512)


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(gen, N, W, dtype=BF16):
    """Seeded CPU normals [N, W] on the GPU, in front of PAD_ROWS NaN rows."""
    buf = torch.full((N + PAD_ROWS, W), float("nan"), dtype=dtype,
                     device="cuda")
    buf[:N] = torch.randn(N, W, generator=gen).to(dtype).cuda()
    out = buf[:N]
    assert out.is_contiguous()
    return out


def _vec(gen, W):
    return torch.randn(W, generator=gen).to(BF16).cuda()


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(_bits(a), _bits(b))


def _assert_colsum(got32, got16, terms64, name):
    """Per column: |got - sum64| <= 1e-4 * sum_rows|term| + 1e-6, and for the
    bf16 result half a bf16 ulp of the value on top.

    Derived, not measured: fp32 sequential accumulation of n terms is off by
    at most n*u*sum|t|; n <= 1025 and u = 6e-8 give 6.2e-5, rounded up to
    1e-4 (the bound of test_kernel_edges_gpu.py, which stops at n = 513).
    The three fp32 roundings inside a dy*xhat term add 3*u*sum|t|, far inside
    the rounding-up.  A missing or doubled row moves a column by |t_row| ~ 1.
    bf16 keeps 8 significant bits, so its ulp at v is at most 2^-7 |v| and
    rounding v to nearest moves it by at most half of that, 2^-8 |v|."""
    assert got32.dtype == F32 and got16.dtype == BF16
    assert torch.isfinite(got32).all() and torch.isfinite(got16).all(), name
    want = terms64.sum(0)
    bound = 1e-4 * terms64.abs().sum(0) + 1e-6
    worst32 = ((got32.double() - want).abs() / bound).max().item()
    bound16 = bound + 2.0 ** -8 * (want.abs() + bound)
    worst16 = ((got16.double() - want).abs() / bound16).max().item()
    print(f"{name}: worst err/bound = {worst32:.3g} (fp32), "
          f"{worst16:.3g} (bf16)")
    assert worst32 <= 1.0, (name, worst32)
    assert worst16 <= 1.0, (name, worst16)
    # the bf16 result is the fp32 one rounded to nearest even
    assert torch.equal(got16, got32.to(BF16)), name


# ------------------------------------------------------------------ LayerNorm

# H: one thread only / idle threads / exactly one trip / thread 0 alone in
# the second trip / the model width / two full trips, all on the fused
# kernel; then the first width past it and a wide one on the dx + partial
# pair.  N: one stripe / single-row stripes only / one stripe short of
# LN_STRIPES / one row over, so one stripe has two rows / uneven halves.
LN_WIDTHS = [8, 1000, 2048, 2056, 2560, 4096, 4104, 8192]
LN_ROWS = [1, 3, 513, LN_STRIPES - 1, LN_STRIPES + 1]


def _ln_case(N, H, with_dh, seed=200):
    g = _gen(seed)
    x, dy = _rows(g, N, H), _rows(g, N, H)
    dh = _rows(g, N, H) if with_dh else None
    w = _vec(g, H)
    x64 = x.double()
    stats = torch.full((2, N + PAD_ROWS), float("nan"), device="cuda")
    mean, rstd = stats[0, :N], stats[1, :N]
    mean.copy_(x64.mean(-1))
    rstd.copy_(torch.rsqrt(x64.var(-1, unbiased=False) + EPS))
    return x, dy, dh, w, mean, rstd


def _ln_call(ext, case, dtype=None):
    x, dy, dh, w, mean, rstd = case
    extra = () if dtype is None else (dtype,)
    if dh is None:
        return ext.layer_norm_bwd(dy, x, w, mean, rstd, *extra)
    return ext.add_layer_norm_bwd(dy, dh, x, w, mean, rstd, *extra)


@pytest.mark.parametrize("with_dh", [False, True], ids=["plain", "dh"])
@pytest.mark.parametrize("H", LN_WIDTHS)
@pytest.mark.parametrize("N", LN_ROWS)
def test_layer_norm_bwd(ext, N, H, with_dh):
    case = _ln_case(N, H, with_dh)
    x, dy, dh, w, mean, rstd = case
    dx, dw, db = _ln_call(ext, case)
    dx16, dw16, db16 = _ln_call(ext, case, BF16)
    dx32, dw32, db32 = _ln_call(ext, case, F32)

    # the kernel was fed these fp32 statistics; the oracle uses the same
    mean64, rstd64 = mean.double(), rstd.double()
    dy64, x64 = dy.double(), x.double()
    dx64, _, _ = ref.layer_norm_bwd(dy64, x64, w.double(), mean64, rstd64)
    if with_dh:
        dx64 = dx64 + dh.double()
    assert torch.isfinite(dx).all()
    torch.testing.assert_close(dx.double(), dx64, rtol=3e-2, atol=3e-2)
    xhat64 = (x64 - mean64.unsqueeze(-1)) * rstd64.unsqueeze(-1)
    _assert_colsum(dw, dw16, dy64 * xhat64, "dw")
    _assert_colsum(db, db16, dy64, "db")

    # the default is fp32, and the same call gives the same bits
    for a, b in ((dx, dx16), (dx, dx32), (dw, dw32), (db, db32)):
        assert _same_bits(a, b)
    for a, b in zip(_ln_call(ext, case, BF16), (dx16, dw16, db16)):
        assert _same_bits(a, b)


# ------------------------------------------------------------------ bias+GeLU

# one thread / a narrow width with idle threads / a second, partial column
# block / the fc1 width, 513 rows spread unevenly over its 409 stripes / one
# row more than stripes there, so one stripe has two rows
GELU_SHAPES = [(1, 8), (3, 1000), (70, 2056), (513, 10240), (410, 10240)]


def test_gelu_shapes_sit_at_the_stripe_count():
    assert gelu_stripes(513, 10240) == 409 == gelu_stripes(410, 10240)


@pytest.mark.parametrize("N,F", GELU_SHAPES)
def test_bias_gelu_bwd(ext, N, F):
    g = _gen(210)
    x, dy = _rows(g, N, F), _rows(g, N, F)
    bias = _vec(g, F)
    dx, db = ext.bias_gelu_bwd(dy, x, bias)
    dx16, db16 = ext.bias_gelu_bwd(dy, x, bias, BF16)
    dx64, _ = ref.bias_gelu_bwd(dy.double(), x.double(), bias.double())
    assert torch.isfinite(dx).all()
    torch.testing.assert_close(dx.double(), dx64, rtol=2e-2, atol=2e-2)
    # the kernel sums the rounded dx it stored
    _assert_colsum(db, db16, dx.double(), "dbias")
    assert _same_bits(dx, dx16)
    for a, b in zip(ext.bias_gelu_bwd(dy, x, bias, BF16), (dx16, db16)):
        assert _same_bits(a, b)
    # and that sum is the column sum of dx, stripe for stripe
    assert _same_bits(db, ext.colsum_bf16(dx))


@pytest.mark.parametrize("N,F", [(1, 8), (3, 10), (70, 100), (513, 2056)])
def test_colsum_out_dtype(ext, N, F):
    t = _rows(_gen(220), N, F)
    got = ext.colsum_bf16(t)
    got16 = ext.colsum_bf16(t, BF16)
    _assert_colsum(got, got16, t.double(), "colsum")
    assert _same_bits(got, ext.colsum_bf16(t, F32))
    assert _same_bits(got16, ext.colsum_bf16(t, BF16))


# -------------------------------------------------------------------- autograd

def test_autograd_grads_are_the_binding_results(ext):
    """ops.* hand autograd the vectors the entries reduced, in the parameter
    dtype, with no cast in between."""
    N, H, F = 70, 1000, 2056
    g = _gen(230)
    x, dy, dh, delta = (_rows(g, N, H) for _ in range(4))
    w, b = _vec(g, H).requires_grad_(), _vec(g, H).requires_grad_()

    y = ops.layer_norm(x, w, b, EPS)
    dw, db = torch.autograd.grad(y, (w, b), dy)
    _, mean, rstd = ext.layer_norm_fwd(x, w, b, EPS)
    _, dw_e, db_e = ext.layer_norm_bwd(dy, x, w, mean, rstd, BF16)
    assert _same_bits(dw, dw_e) and _same_bits(db, db_e)

    h, y = ops.add_layer_norm(x, delta, w, b, EPS)
    dw, db = torch.autograd.grad((h, y), (w, b), (dh, dy))
    h_e, _, mean, rstd = ext.add_layer_norm_fwd(x, delta, w, b, EPS)
    _, dw_e, db_e = ext.add_layer_norm_bwd(dy, dh, h_e, w, mean, rstd, BF16)
    assert _same_bits(dw, dw_e) and _same_bits(db, db_e)

    gx, gdy = _rows(g, N, F), _rows(g, N, F)
    gb = _vec(g, F).requires_grad_()
    (dgb,) = torch.autograd.grad(ops.bias_gelu(gx, gb), (gb,), gdy)
    assert _same_bits(dgb, ext.bias_gelu_bwd(gdy, gx, gb, BF16)[1])

    lw = _rows(g, F, H)
    (dlb,) = torch.autograd.grad(ops.linear_bias(x, lw, gb), (gb,), gdy)
    assert _same_bits(dlb, ext.colsum_bf16(gdy, BF16))


# --------------------------------------------------------------- graph capture

def test_backwards_replay_from_a_captured_graph(ext):
    N, H, F = 70, 2560, 2056
    case = _ln_case(N, H, True, seed=240)
    x, dy, dh, w, mean, rstd = case
    g = _gen(241)
    gx, gdy, gb = _rows(g, N, F), _rows(g, N, F), _vec(g, F)

    def run():
        return (*ext.layer_norm_bwd(dy, x, w, mean, rstd, BF16),
                *ext.add_layer_norm_bwd(dy, dh, x, w, mean, rstd, BF16),
                *ext.bias_gelu_bwd(gdy, gx, gb, BF16),
                ext.colsum_bf16(gdy, BF16))

    eager = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert _same_bits(got, want)


# ------------------------------------------------------------------- refusals

def _z(*shape, dtype=BF16):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def _refusal_calls():
    n, h = 4, 16
    st = lambda: _z(n, dtype=F32)  # noqa: E731
    return {
        "layer_norm_bwd": lambda e, d: e.layer_norm_bwd(
            _z(n, h), _z(n, h), _z(h), st(), st(), d),
        "add_layer_norm_bwd": lambda e, d: e.add_layer_norm_bwd(
            _z(n, h), _z(n, h), _z(n, h), _z(h), st(), st(), d),
        "bias_gelu_bwd": lambda e, d: e.bias_gelu_bwd(
            _z(n, h), _z(n, h), _z(h), d),
        "colsum_bf16": lambda e, d: e.colsum_bf16(_z(n, h), d),
    }


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.int32],
                         ids=str)
@pytest.mark.parametrize("entry", sorted(_refusal_calls()))
def test_out_dtype_is_refused(ext, entry, dtype):
    """Only fp32 and bf16 come out of the finalize kernel; anything else is
    refused by name before an allocation or a launch.  The operands are
    valid, so the call would stay inside its buffers anyway."""
    with pytest.raises(RuntimeError, match=r"(^|\W)out_dtype(\W|$)") as info:
        _refusal_calls()[entry](ext, dtype)
    assert "HIP error" not in str(info.value)


@pytest.mark.parametrize("entry", sorted(_refusal_calls()))
def test_out_dtype_does_not_relax_operand_checks(ext, entry):
    """With out_dtype given, a short bias / w / width-0 operand is still
    refused by its own name."""
    n, h = 4, 16
    st = _z(n, dtype=F32)
    calls = {
        "layer_norm_bwd": ("w", lambda: ext.layer_norm_bwd(
            _z(n, h), _z(n, h), _z(h + 8), st, st, BF16)),
        "add_layer_norm_bwd": ("dh", lambda: ext.add_layer_norm_bwd(
            _z(n, h), _z(n + 1, h), _z(n, h), _z(h), st, st, BF16)),
        "bias_gelu_bwd": ("bias", lambda: ext.bias_gelu_bwd(
            _z(n, h), _z(n, h), _z(h + 8), BF16)),
        "colsum_bf16": ("t", lambda: ext.colsum_bf16(_z(n, 0), BF16)),
    }
    name, call = calls[entry]
    with pytest.raises(RuntimeError,
                       match=rf"(^|\W){name}(\W|$)") as info:
        call()
    assert "HIP error" not in str(info.value)
