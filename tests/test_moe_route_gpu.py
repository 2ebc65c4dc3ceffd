"""Fused top-2 MoE routing, dispatch and combine kernels (gfx950) against
the fixed-shape fp32 reference, and ExpertParallelMLP on the fused path
against its torch-op path.

Shapes are the smallest at which the scan, the tails or the vector path
can go wrong: N in {1, 63, 64, 65, 257, 1000} (partial wave, wave boundary,
block boundary, four blocks with a tail), E in {2, 3, 8, 64, 128},
H in {8, 264, 1024}."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from moe_route_utils import (assert_top3_distinct, check_invariants,
                             tie_free_logits)

from alpa_amd import ops
from alpa_amd.global_env import global_config
from alpa_amd.ops import reference as ref
from alpa_amd.parallel.expert import ExpertParallelMLP

BF16 = torch.bfloat16
# fp32 chain of five or so ops plus a hardware exp
ROUTE_TOL = dict(rtol=1e-4, atol=1e-6)


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _routing(ext, logits, C):
    """(MoERouting, count1) straight from the extension."""
    out = ext.moe_route_fwd(logits, C)
    return ops.MoERouting(*out[:8]), out[8]


def _ref_routing(logits, C):
    """The fp32 CPU reference on the same bf16 values."""
    out = ref.moe_top2_route(logits.float().cpu(), C)
    return ops.MoERouting(*out[:8]), out[8]


def _assert_route_matches(ext, logits, C):
    N, E = logits.shape
    got, count1 = _routing(ext, logits, C)
    want, want_count1 = _ref_routing(logits, C)
    for name in ("idx1", "idx2", "slot1", "slot2", "src"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == torch.int32
        assert torch.equal(g.cpu(), w), (name, N, E, C)
    assert torch.equal(count1.cpu(), want_count1)
    for name in ("w1", "w2", "aux_loss"):
        g, w = getattr(got, name).cpu(), getattr(want, name)
        print(f"N={N} E={E} C={C} {name}: max rel err "
              f"{float(((g - w).abs() / w.abs().clamp_min(1e-30)).max()):.3g}")
        torch.testing.assert_close(g, w, **ROUTE_TOL)
    check_invariants(got, N, E, C)
    return got


# (N, E, C): C = 1 drops first choices, small C drops both kinds with the
# min(count1, C) base active, large C drops nothing
ROUTE_CASES = [(1, 2, 1), (1, 128, 3), (63, 3, 42), (64, 8, 16),
               (65, 64, 2), (257, 128, 4), (257, 2, 300), (1000, 3, 1),
               (1000, 8, 250), (1000, 64, 7), (1000, 128, 16)]


@pytest.mark.parametrize("N,E,C", ROUTE_CASES)
def test_route_matches_reference(ext, N, E, C):
    logits = tie_free_logits(N, E, seed=N * 131 + E, dtype=BF16)
    assert_top3_distinct(logits)
    _assert_route_matches(ext, logits.cuda(), C)


@pytest.mark.parametrize("N,E", [(65, 8), (257, 8), (1000, 64)])
def test_route_skewed_matches_reference(ext, N, E):
    """+8 on one column: every token wants expert 2 first, so both choices
    drop and second choices queue behind min(count1, C)."""
    logits = tie_free_logits(N, E, seed=N + E)
    logits[:, 2] += 8.0
    logits = logits.to(BF16)
    assert torch.equal(logits.float()[:, 2],
                       tie_free_logits(N, E, seed=N + E)[:, 2] + 8.0)
    assert_top3_distinct(logits)
    for C in (1, max(1, 2 * N // E)):
        got = _assert_route_matches(ext, logits.cuda(), C)
        assert int((got.slot1 < 0).sum()) == N - C
        assert int((got.idx1 != 2).sum()) == 0


@pytest.mark.parametrize("N,E", [(257, 8), (1000, 64)])
def test_route_mild_skew_matches_reference(ext, N, E):
    """+0.5 on one column: expert 2 is the first choice of many tokens and
    the second choice of most others, so second choices for it queue
    behind a full min(count1, C) base and drop.  The shifted column ties
    with others; both sides break ties the same way."""
    logits = tie_free_logits(N, E, seed=N + E)
    logits[:, 2] += 0.5
    logits = logits.to(BF16)
    C = max(1, N // E)
    got = _assert_route_matches(ext, logits.cuda(), C)
    second_to_2 = got.idx2 == 2
    assert int(second_to_2.sum()) > 0
    assert int((got.idx1 == 2).sum()) > C
    assert bool((got.slot2[second_to_2] < 0).all())


@pytest.mark.parametrize("N,E,C", [(63, 3, 20), (1000, 64, 20)])
def test_route_with_ties_matches_reference(ext, N, E, C):
    """Coarse logits full of exact ties: the lowest index must win in the
    kernel as in the reference."""
    logits = torch.randint(-2, 3, (N, E), generator=_gen(N)).to(BF16) / 2
    _assert_route_matches(ext, logits.cuda(), C)


def test_route_empty_batch(ext):
    out = ext.moe_route_fwd(torch.empty(0, 4, dtype=BF16, device="cuda"), 3)
    assert [tuple(t.shape) for t in out] == [(0,)] * 6 + [(12,), (), (4,)]
    assert bool((out[6] == -1).all()) and float(out[7]) == 0.0


@pytest.mark.parametrize("N,E,C", [(1, 2, 1), (65, 3, 30), (257, 128, 4),
                                   (1000, 8, 100)])
def test_route_backward_matches_autograd(N, E, C):
    g = _gen(N + E)
    logits = torch.randn(N, E, generator=g).to(BF16)
    dw1, dw2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    daux = torch.randn((), generator=g)

    lg = logits.cuda().requires_grad_(True)
    r = ops.moe_top2_route(lg, C)
    got, = torch.autograd.grad((r.w1, r.w2, r.aux_loss), lg,
                               (dw1.cuda(), dw2.cuda(), daux.cuda()))
    assert got.dtype == BF16

    lr = logits.float().requires_grad_(True)
    w1, w2, *_, aux, _c = ref.moe_top2_route(lr, C)
    want, = torch.autograd.grad((w1, w2, aux), lr, (dw1, dw2, daux))
    # one bf16 rounding on each side
    torch.testing.assert_close(got.float().cpu(), want.to(BF16).float(),
                               rtol=2.0 ** -7, atol=1e-6)


# (N, E, C, H)
MOVE_CASES = [(1, 2, 1, 8), (65, 3, 30, 264), (64, 128, 1, 8),
              (257, 8, 40, 1024), (1000, 64, 20, 264)]


def _move_inputs(ext, N, E, C, H):
    g = _gen(N * 7 + H)
    logits = torch.randn(N, E, generator=g).to(BF16).cuda()
    r, _ = _routing(ext, logits, C)
    rc = ops.MoERouting(*[t.cpu() for t in r])
    x = torch.randn(N, H, generator=g).to(BF16)
    y = torch.randn(E * C, H, generator=g).to(BF16)
    return g, r, rc, x, y


@pytest.mark.parametrize("N,E,C,H", MOVE_CASES)
def test_dispatch_forward_backward(ext, N, E, C, H):
    g, r, rc, x, y = _move_inputs(ext, N, E, C, H)
    xg = x.cuda().requires_grad_(True)
    out = ops.moe_dispatch(xg, r)
    assert torch.equal(out.cpu(), ref.moe_dispatch(x, rc.src))
    gy = torch.randn(E * C, H, generator=g).to(BF16)
    dx, = torch.autograd.grad(out, xg, gy.cuda())
    # a sum of at most two bf16 values in fp32, rounded once
    torch.testing.assert_close(
        dx.cpu().float(),
        ref.moe_dispatch_bwd(gy, rc.slot1, rc.slot2).float(),
        rtol=2.0 ** -8, atol=0.0)


@pytest.mark.parametrize("N,E,C,H", MOVE_CASES)
def test_combine_forward_backward(ext, N, E, C, H):
    g, r, rc, x, y = _move_inputs(ext, N, E, C, H)
    yg = y.cuda().requires_grad_(True)
    w1g = r.w1.detach().requires_grad_(True)
    w2g = r.w2.detach().requires_grad_(True)
    out = ops.moe_combine(yg, r._replace(w1=w1g, w2=w2g))
    # fp32 reference on the same bf16 values; the kernel rounds once
    want = ref.moe_combine(y.float(), rc.w1, rc.w2, rc.slot1, rc.slot2)
    torch.testing.assert_close(out.cpu().float(), want, rtol=2.0 ** -8,
                               atol=1e-5 * float(y.float().abs().max()))

    dout = torch.randn(N, H, generator=g).to(BF16)
    dy, dw1, dw2 = torch.autograd.grad(out, (yg, w1g, w2g), dout.cuda())
    want_dy, want_dw1, want_dw2 = ref.moe_combine_bwd(
        dout.float(), y.float(), rc.w1, rc.w2, rc.slot1, rc.slot2, rc.src)
    torch.testing.assert_close(dy.cpu().float(), want_dy, rtol=2.0 ** -8,
                               atol=1e-5 * float(dout.float().abs().max()))
    # fp32 dots over H <= 1024 of randn data
    torch.testing.assert_close(dw1.cpu(), want_dw1, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(dw2.cpu(), want_dw2, rtol=1e-3, atol=1e-3)
    assert bool((dw1.cpu()[rc.slot1 < 0] == 0).all())
    assert bool((dw2.cpu()[rc.slot2 < 0] == 0).all())


def test_dispatch_combine_past_2_31_elements(ext):
    """Row offsets beyond 2^31 elements: the last expert's slots start at
    3*C*H = 2.15e9.  Eight tokens, so nearly every row is a zero row."""
    N, E, C, H = 8, 4, 700000, 1024
    assert (E - 1) * C * H > 2 ** 31
    logits = torch.full((N, E), -4.0)
    t = torch.arange(N)
    logits[t, t % E] = 2.0              # first choice t % 4
    logits[t, (t + 1) % E] = 1.0        # second choice (t + 1) % 4
    r, _ = _routing(ext, logits.to(BF16).cuda(), C)
    check_invariants(r, N, E, C)
    x = torch.randn(N, H, generator=_gen(0)).to(BF16).cuda()
    out = ops.moe_dispatch(x, r)
    assert out.shape == (E * C, H)
    s1, s2 = r.slot1.long(), r.slot2.long()
    assert int(s1.max()) >= (E - 1) * C
    assert torch.equal(out[s1], x) and torch.equal(out[s2], x)
    assert int((out != 0).any(-1).sum()) == 2 * N
    back = ops.moe_combine(out, r)      # w1*x + w2*x, w1 + w2 = 1
    torch.testing.assert_close(back.float(), x.float(), rtol=2.0 ** -7,
                               atol=0.0)


def test_hostile_rows(ext):
    """A NaN row, a +inf row and an all -inf row among 65: routing stays
    structurally valid, the other rows are untouched, and dispatch and
    combine run on the resulting slots."""
    N, E, C, H = 65, 8, 9, 264
    logits = tie_free_logits(N, E, seed=5, dtype=BF16)
    bad = [7, 33, 64]
    logits[7, 3] = float("nan")
    logits[33, 5] = float("inf")
    logits[64] = float("-inf")
    got, count1 = _routing(ext, logits.cuda(), C)
    check_invariants(got, N, E, C)
    want, want_count1 = _ref_routing(logits, C)
    # the reference scans with the same NaN rule, so even these agree
    for name in ("idx1", "idx2", "slot1", "slot2", "src"):
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name))
    assert torch.equal(count1.cpu(), want_count1)
    ok = torch.ones(N, dtype=torch.bool)
    ok[bad] = False
    torch.testing.assert_close(got.w1.cpu()[ok], want.w1[ok], **ROUTE_TOL)
    torch.testing.assert_close(got.w2.cpu()[ok], want.w2[ok], **ROUTE_TOL)

    g = _gen(1)
    x = torch.randn(N, H, generator=g).to(BF16).cuda().requires_grad_(True)
    disp = ops.moe_dispatch(x, got)
    out = ops.moe_combine(disp * 2, got)
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(disp).all())
    assert bool(torch.isfinite(out.cpu()[ok]).all())
    assert bool(torch.isfinite(x.grad.cpu()[ok]).all())


def test_deterministic(ext):
    N, E, C, H = 1000, 8, 100, 264
    g = _gen(3)
    logits = torch.randn(N, E, generator=g).to(BF16).cuda()
    x0 = torch.randn(N, H, generator=g).to(BF16).cuda()
    gout = torch.randn(N, H, generator=g).to(BF16).cuda()

    def run():
        lg = logits.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        r = ops.moe_top2_route(lg, C)
        disp = ops.moe_dispatch(x, r)
        out = ops.moe_combine(torch.tanh(disp), r)
        loss = (out.float() * gout.float()).sum() + r.aux_loss
        grads = torch.autograd.grad(loss, (lg, x))
        return (*r, disp, out, *grads)

    first, second = run(), run()
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i


def _mlp(capacity_factor=2.0, hidden=64, ffn=128, E=4, dtype=BF16):
    return ExpertParallelMLP(hidden, ffn, E, None, 1,
                             capacity_factor=capacity_factor, dtype=dtype,
                             device="cuda")


def _with_fused(flag, fn):
    old = global_config.moe_fused_routing
    global_config.moe_fused_routing = flag
    try:
        return fn()
    finally:
        global_config.moe_fused_routing = old


def test_module_fused_path_never_syncs():
    m = _mlp()
    x = torch.randn(2, 32, 64, generator=_gen(0)).to(BF16).cuda() \
        .requires_grad_(True)
    assert ops.moe_fused_ok(x.reshape(64, 64), 4)

    def step():
        m(x).float().square().mean().backward()

    _with_fused(True, step)             # warm up outside the checked region
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.nonzero(torch.ones(4, device="cuda"))
            control = False
        except RuntimeError:
            control = True
        if control:
            _with_fused(True, step)
            with pytest.raises(RuntimeError):
                _with_fused(False, step)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not control:
        pytest.skip("sync debug mode does not flag torch.nonzero on this "
                    "build")


@pytest.mark.parametrize("capacity_factor", [8.0, 0.5])
def test_module_fused_matches_unfused(capacity_factor):
    m = _mlp(capacity_factor)
    # topk in the unfused path has no defined tie order: take the first
    # seed whose gate logits have pairwise distinct top-3 in every row
    for seed in range(50):
        x = torch.randn(2, 32, 64, generator=_gen(seed)).to(BF16).cuda()
        logits = x.reshape(64, 64) @ m.wg
        top = logits.float().topk(3, dim=-1).values
        if bool((top[:, :-1] > top[:, 1:]).all()):
            break
    assert_top3_distinct(logits)
    gout = torch.randn(2, 32, 64, generator=_gen(99)).cuda()
    x.requires_grad_(True)
    params = (x, m.wg, m.w1, m.w2)

    def run():
        y = m(x)
        aux = m.last_aux_loss
        grads = torch.autograd.grad((y.float() * gout).sum() + aux, params)
        return y, aux, grads

    y_f, aux_f, g_f = _with_fused(True, run)
    y_u, aux_u, g_u = _with_fused(False, run)
    C = max(1, int(capacity_factor * 64 * 2 / 4))
    dropped = int((ops.moe_top2_route(logits, C).slot2 < 0).sum())
    assert (dropped > 0) == (capacity_factor < 1)
    torch.testing.assert_close(aux_f, aux_u, rtol=1e-4, atol=0.0)
    # the unfused combine rounds three times where the fused one rounds once
    torch.testing.assert_close(y_f.float(), y_u.float(), rtol=2e-2, atol=2e-2)
    for name, a, b in zip(("x", "wg", "w1", "w2"), g_f, g_u):
        rel = float((a.float() - b.float()).norm() / b.float().norm())
        print(f"cf={capacity_factor} grad {name}: rel L2 {rel:.3g}")
        assert rel <= 3e-2, (name, rel)


def test_envelope_falls_back_to_torch_ops():
    assert not ops.moe_fused_ok(torch.zeros(64, 64, device="cuda"), 4)
    assert not ops.moe_fused_ok(
        torch.zeros(64, 12, dtype=BF16, device="cuda"), 4)
    assert not ops.moe_fused_ok(
        torch.zeros(64, 64, dtype=BF16, device="cuda"), 129)
    assert not ops.moe_fused_ok(
        torch.zeros(64, 64, dtype=BF16, device="cuda"), 4, 2 ** 29)
    assert ops.moe_fused_ok(
        torch.zeros(64, 64, dtype=BF16, device="cuda"), 4, 32)

    # fp32 on the GPU: the old path, checked against the same weights on
    # the CPU
    m = _mlp(dtype=torch.float32)
    ref_m = ExpertParallelMLP(64, 128, 4, None, 1, capacity_factor=2.0)
    ref_m.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    x = torch.randn(2, 32, 64, generator=_gen(4))
    torch.testing.assert_close(m(x.cuda()).cpu(), ref_m(x), rtol=1e-3,
                               atol=1e-4)
    torch.testing.assert_close(m.last_aux_loss.cpu(), ref_m.last_aux_loss,
                               rtol=1e-4, atol=0.0)

    # H = 12 and E = 129 in bf16: still the old path, still a sane result
    for hidden, E in ((12, 4), (64, 129)):
        mm = _mlp(hidden=hidden, ffn=16, E=E)
        xx = torch.randn(2, 32, hidden, generator=_gen(5)).to(BF16).cuda()
        out = mm(xx)
        assert out.shape == xx.shape and bool(torch.isfinite(out).all())
        assert float(out.detach().float().abs().sum()) > 0
