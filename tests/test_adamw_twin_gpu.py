"""The tiled path of the multi-tensor AdamW kernel, which also writes each
parameter's transposed twin.

Every case runs three steps twice on cloned inputs, once with twins and once
without (the flat path), and asks for bit-identical p, m and v and for a twin
that is bit-identical to p.t().  Both runs use the same element update, so
nothing may differ.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd import ops

BF16 = torch.bfloat16
T = ops._ADAM_TILE
STEPS = 3
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), what


def _make(shapes, dtypes=None, seed=0):
    """(p, g, m, v) lists on the GPU; m and v start non-zero."""
    gen = torch.Generator().manual_seed(seed)
    dtypes = dtypes or [BF16] * len(shapes)
    p = [torch.randn(s, generator=gen).to(dt).cuda()
         for s, dt in zip(shapes, dtypes)]
    g = [torch.randn(s, generator=gen).to(dt).cuda()
         for s, dt in zip(shapes, dtypes)]
    m = [(0.1 * torch.randn(s, generator=gen)).cuda() for s in shapes]
    v = [(0.1 * torch.rand(s, generator=gen)).cuda() for s in shapes]
    return p, g, m, v


def _twins_for(p, want):
    """A twin (filled with p.t()) where `want` says so and the Python layer
    agrees, else None."""
    return [x.t().contiguous() if w and ops.weight_twin_eligible(x) else None
            for x, w in zip(p, want)]


def _clone(ts):
    return [t.clone() for t in ts]


def _run_both(p, g, m, v, twins, check_each_step=None, **kw):
    """Three steps with twins and three without on clones; compares after
    every step.  Returns the twinned run's (p, m, v, twins)."""
    pa, ma, va = _clone(p), _clone(m), _clone(v)
    pb, mb, vb = _clone(p), _clone(m), _clone(v)
    for step in range(1, STEPS + 1):
        ops.fused_adamw(pa, g, ma, va, step, twins=twins, **HYPER, **kw)
        ops.fused_adamw(pb, g, mb, vb, step, **HYPER, **kw)
        torch.cuda.synchronize()
        for i in range(len(p)):
            _same(pa[i], pb[i], f"p[{i}] step {step}")
            _same(ma[i], mb[i], f"m[{i}] step {step}")
            _same(va[i], vb[i], f"v[{i}] step {step}")
            if twins[i] is not None:
                _same(twins[i], pa[i].t().contiguous(),
                      f"twin[{i}] step {step}")
    return pa, ma, va, twins


@pytest.mark.parametrize("shape", [(T, T), (2 * T, 3 * T), (256, 320)])
def test_single_tensor(shape):
    p, g, m, v = _make([shape])
    twins = _twins_for(p, [True])
    assert twins[0] is not None
    pa, _, _, _ = _run_both(p, g, m, v, twins)
    assert not torch.equal(pa[0], p[0])  # the steps did move the parameter


def test_mixed_list_and_forced_twin_is_rejected():
    shapes = [(2 * T, T), (T, 2 * T), (3 * T,), (T, T), (T + 8, T)]
    dtypes = [BF16, BF16, BF16, torch.float32, BF16]
    p, g, m, v = _make(shapes, dtypes, seed=1)
    # twinned 2-D, untwinned 2-D, bias, fp32, dims that are no tile multiple
    twins = _twins_for(p, [True, False, True, True, True])
    assert [t is not None for t in twins] == [True, False, False, False,
                                              False]
    _run_both(p, g, m, v, twins)
    # the binding refuses a twin forced on what the Python layer turned down
    odd = p[4]
    with pytest.raises(RuntimeError, match="multiples of"):
        ops.fused_adamw([odd.clone()], [g[4]], [m[4].clone()], [v[4].clone()],
                        1, twins=[odd.t().contiguous()], **HYPER)
    with pytest.raises(RuntimeError, match="twin"):
        ops.fused_adamw([p[0].clone()], [g[0]], [m[0].clone()],
                        [v[0].clone()], 1,
                        twins=[p[0].clone()], **HYPER)  # [rows, cols]


def test_grad_view_at_odd_offset():
    """g as a bucket view that is not 16-byte aligned."""
    shape = (2 * T, 2 * T)
    p, g, m, v = _make([shape], seed=2)
    flat = torch.zeros(shape[0] * shape[1] + 8, dtype=BF16, device="cuda")
    for off in (1, 3):
        view = flat[off:off + g[0].numel()].view(shape)
        view.copy_(g[0])
        assert view.data_ptr() % 16 != 0
        _run_both(p, [view], m, v, _twins_for(p, [True]))


def test_clipping_finite_norm():
    p, g, m, v = _make([(T, 2 * T), (T,)], seed=3)
    sumsq = ops.multi_tensor_sumsq(g)
    norm = float(sumsq.sqrt())
    pa, _, _, _ = _run_both(p, g, m, v, _twins_for(p, [True, False]),
                            grad_sumsq=sumsq, max_grad_norm=0.5 * norm)
    assert not torch.equal(pa[0], p[0])


def test_clipping_inf_gradient_changes_nothing():
    p, g, m, v = _make([(T, 2 * T), (T,)], seed=4)
    g[0][3, 5] = float("inf")
    sumsq = ops.multi_tensor_sumsq(g)
    assert not torch.isfinite(sumsq).all()
    twins = _twins_for(p, [True, False])
    pa, ma, va, twins = _run_both(p, g, m, v, twins, grad_sumsq=sumsq,
                                  max_grad_norm=1.0)
    _same(pa[0], p[0], "p untouched")
    _same(ma[0], m[0], "m untouched")
    _same(va[0], v[0], "v untouched")
    _same(twins[0], p[0].t().contiguous(), "twin untouched")


def test_grad_scale():
    p, g, m, v = _make([(2 * T, T)], seed=5)
    _run_both(p, g, m, v, _twins_for(p, [True]), grad_scale=-0.125)


def test_graph_capture_three_replays():
    p, g, m, v = _make([(2 * T, 2 * T), (T,)], seed=6)
    twins = _twins_for(p, [True, False])
    pa, ma, va = _clone(p), _clone(m), _clone(v)
    pb, mb, vb = _clone(p), _clone(m), _clone(v)
    # bias correction is a launch argument: a captured step replays step 1's
    step = 1
    # builds the cached tables outside capture, on throwaway state
    ops.fused_adamw(pa, g, ma, va, step, twins=twins, **HYPER)
    for dst, src in zip(pa + ma + va, p + m + v):
        dst.copy_(src)
    twins[0].copy_(p[0].t())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fused_adamw(pa, g, ma, va, step, twins=twins, **HYPER)
    torch.cuda.synchronize()
    for dst, src in zip(pa + ma + va, p + m + v):  # capture ran nothing,
        dst.copy_(src)                             # start from the inputs
    for replay in range(3):
        graph.replay()
        ops.fused_adamw(pb, g, mb, vb, step, **HYPER)
        torch.cuda.synchronize()
        for i in range(len(p)):
            _same(pa[i], pb[i], f"p[{i}] replay {replay}")
            _same(ma[i], mb[i], f"m[{i}] replay {replay}")
            _same(va[i], vb[i], f"v[{i}] replay {replay}")
        _same(twins[0], pa[0].t().contiguous(), f"twin replay {replay}")
