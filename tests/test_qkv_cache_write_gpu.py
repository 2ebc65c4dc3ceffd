"""csrc/qkv_cache_write.hip against reference.qkv_cache_write, bit for bit:
q, k_new, the written cache rows and scales, and the sentinel everywhere else.
Every operand is a view: qkv of a wider token buffer, the caches of buffers
one slot and two rows larger.  B = 2, h = 3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd import ops
from alpa_amd.ops import reference as ref

B, H = 2, 3
F32, BF16 = torch.float32, torch.bfloat16
POS = {"int": 2, "i32": [1, 3], "i64": [3, 0]}

# d, rotary_dim, S, pos, e4m3 cache, table dtype, special
CASES = [
    (16, None, 1, "int", False, None, None),
    (16, 8, 3, "i32", False, F32, None),
    (16, 16, 1, "i64", True, BF16, None),
    (16, 16, 3, "int", True, F32, None),
    (80, None, 3, "i64", True, None, None),
    (80, 8, 1, "int", False, BF16, None),
    (80, 80, 3, "i32", False, F32, None),
    (80, 80, 1, "i64", True, F32, None),
    (80, 8, 3, "i32", True, BF16, None),
    (256, None, 1, "i32", False, None, None),
    (256, 8, 3, "i64", False, BF16, None),
    (256, 256, 1, "int", True, F32, None),
    (256, 256, 3, "i32", True, BF16, None),
    (256, 64, 1, "i64", False, F32, None),
    (256, None, 3, "int", True, None, None),
    # slot 1 starts at L: q rows zero, cache untouched; slot 0 is written
    (80, None, 3, "i32", False, None, "past_L"),
    (80, 8, 3, "i64", True, F32, "past_L"),
    # tables shorter than the cache: slot 1 leaves them after one row
    (256, 64, 3, "i32", False, BF16, "past_T"),
    (16, 8, 3, "i64", True, F32, "past_T"),
    # scale 1; scale NaN with 0x7F bytes
    (80, 8, 1, "i32", True, F32, "zero_k"),
    (16, None, 3, "i32", True, None, "zero_k"),
    (256, None, 3, "int", True, None, "nan_v"),
    # 2112 tasks of 32 lanes: past the one-wave-workgroup threshold
    (256, 64, 352, "int", False, F32, None),
    (256, 8, 352, "i64", True, BF16, None),
]


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}
                  [t.element_size()])


def _case(d, rd, S, pos, fp8, tdt, special):
    """CPU base buffers, and `views(buffers, device)` -> the op's operands."""
    gen = torch.Generator().manual_seed(d + S)
    L = S + 5
    T = 5 if special == "past_T" else L + 2
    wide = torch.randn(B, S, 3 * H * d + 16, generator=gen).bfloat16()
    x = wide[:, :, :3 * H * d].view(B, S, H, 3, d)
    if special == "zero_k":
        x[0, 0, 0, 1] = 0
    if special == "nan_v":
        x[1, 0, 1, 2, 3] = float("nan")
    if fp8:
        rows = torch.full((2, B + 1, H, L + 2, d), 0x7F, dtype=torch.uint8)
        scales = torch.full((2, B + 1, H, L + 2), float("nan"))
    else:
        rows = torch.full((2, B + 1, H, L + 2, d), 7.0, dtype=BF16)
        scales = torch.zeros(0)
    at = {"past_L": [1, L], "past_T": [0, 4]}.get(special, POS[pos])
    sin = cos = torch.zeros(0)
    if rd is not None:
        from alpa_amd.models.codegen import rotary_tables
        sin, cos = rotary_tables(rd, T, tdt, "cpu")

    def views(bufs, device):
        wide, rows, scales, sin, cos = bufs
        qkv = wide[:, :, :3 * H * d].view(B, S, H, 3, d)
        c = rows.view(torch.float8_e4m3fn) if fp8 else rows
        ck, cv = c[0, 1:, :, :L], c[1, 1:, :, :L]
        if fp8:
            ck, cv = (ck, scales[0, 1:, :, :L]), (cv, scales[1, 1:, :, :L])
        p = at if pos == "int" else torch.tensor(
            at, dtype=torch.int32 if pos == "i32" else torch.int64,
            device=device)
        rotary = None if rd is None else (sin, cos, rd)
        return qkv, ck, cv, p, rotary

    touched = torch.zeros(B + 1, H, L + 2, dtype=torch.bool)
    for b, p in enumerate([at] * B if isinstance(at, int) else at):
        touched[b + 1, :, p:min(p + S, L, T if rd else L)] = True
    return [wide, rows, scales, sin, cos], views, touched


@pytest.mark.parametrize("d,rd,S,pos,fp8,tdt,special", CASES)
def test_kernel_equals_reference(d, rd, S, pos, fp8, tdt, special):
    bufs, views, touched = _case(d, rd, S, pos, fp8, tdt, special)
    dev = [t.cuda() for t in bufs]
    sentinel = [_bits(bufs[i]).flatten()[0].clone() if bufs[i].numel() else
                None for i in (1, 2)]
    want = ref.qkv_cache_write(*views(bufs, "cpu"), want_k=True)
    args = views(dev, "cuda")
    assert ops.qkv_cache_write_ok(*args)
    got = ops.qkv_cache_write(*args, want_k=S > 1)
    got = got if S > 1 else (got,)
    for g, w in zip(got, want):
        assert g.is_contiguous() and torch.equal(_bits(g.cpu()), _bits(w))
    for i in (1, 2) if fp8 else (1,):
        now = _bits(dev[i].cpu())
        assert torch.equal(now, _bits(bufs[i]))
        assert bool((now[:, ~touched] == sentinel[i - 1]).all())
    if special == "past_L":
        assert bool((got[0][1] == 0).all()) and not touched[2].any()
    if special in ("zero_k", "nan_v"):
        half, b, hd, byte, sc = (0, 0, 0, None, 1.0) if special == "zero_k" \
            else (1, 1, 1, 0x7F, float("nan"))
        p = POS[pos] if pos == "int" else POS[pos][b]
        scale = float(dev[2][half, b + 1, hd, p])
        assert scale == sc or (sc != sc and scale != scale)
        if byte is not None:
            assert bool((dev[1][half, b + 1, hd, p] == byte).all())


def _good():
    d, S, L = 16, 2, 8
    qkv = torch.randn(B, S, H, 3, d, device="cuda").bfloat16()
    ck, cv = (torch.zeros(B, H, L, d, device="cuda", dtype=BF16)
              for _ in range(2))
    sin, cos = (torch.zeros(L, 4, device="cuda") for _ in range(2))
    return dict(qkv=qkv, cache_k=ck, cache_v=cv, pos=2, sin=sin, cos=cos,
                rotary_dim=8)


def _fp16(a):
    a["qkv"] = a["qkv"].half()


def _row_stride(a):
    a["qkv"] = torch.zeros(B, 2, H, 3, 24, device="cuda", dtype=BF16)[..., :16]


def _misaligned(a):
    flat = torch.zeros(a["qkv"].numel() + 8, device="cuda", dtype=BF16)
    a["qkv"] = flat[4:-4].view_as(a["qkv"])


def _rotary_12(a):
    a["sin"], a["cos"], a["rotary_dim"] = a["sin"][:, :3].contiguous() \
        .repeat(1, 2), a["cos"][:, :3].contiguous().repeat(1, 2), 12


def _short_tables(a):
    a["sin"], a["cos"] = a["sin"][:3].contiguous(), a["cos"][:3].contiguous()


def _heads(a):
    a["cache_k"] = torch.zeros(B, H + 1, 8, 16, device="cuda", dtype=BF16)


@pytest.mark.parametrize("breaker,message", [
    (_fp16, "qkv must be bf16"), (_row_stride, "head_dim apart"),
    (_misaligned, "16-byte aligned"), (_rotary_12, "multiple of 8"),
    (_short_tables, "outside the rotary tables"), (_heads, "size 3 in dim"),
])
def test_binding_refuses(breaker, message):
    from alpa_amd.ops._backend import hip_ops
    args = _good()
    hip_ops().qkv_cache_write(**args)
    breaker(args)
    with pytest.raises(RuntimeError, match=message):
        hip_ops().qkv_cache_write(**args)
