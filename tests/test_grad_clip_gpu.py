"""Global-norm gradient clipping on the gfx950 kernels: the multi-tensor sum
of squares, its finalize, and the clipped multi-tensor AdamW step.

The shapes are those of the AdamW edge test (tests/test_kernel_edges_gpu.py,
copied here): vector-width tails, chunk boundaries, more than one chunk,
views that are not 16-byte aligned, plus a list long enough that the
finalize kernel meets more partials than it has threads.  The oracle is
alpa_amd.ops.reference on fp64 copies of the inputs.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd.ops import reference as ref

BF16 = torch.bfloat16

ADAM_BF16_NUMELS = [1, 7, 8, 9, 16383, 16384, 16385, 2 * 16384 + 13]
ADAM_FP32_NUMELS = [5, 16385]
ADAM_GUARD = 64          # sentinel elements on each side of every tensor
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-2, 0.9, 0.95, 1e-8
ADAM_STEPS = (1, 2, 1000)
FILL = 1234.5

# Views that are NOT 16-byte aligned, as (dtype, numel, element offsets of
# p, g, m, v past an aligned base).  Gradient offsets 3, 5 and 7 (bf16) and
# 1 and 2 (fp32) send the sum of squares down its element-wise path.
ADAM_MISALIGNED = [
    (BF16, 5, (3, 3, 0, 0)),
    (BF16, 16385, (3, 3, 0, 0)),
    (BF16, 2 * 16384 + 13, (7, 7, 0, 0)),
    (torch.float32, 3, (1, 1, 0, 0)),
    (torch.float32, 16384 + 9, (1, 1, 0, 0)),
    (BF16, 16384 + 9, (4, 4, 4, 4)),
    (torch.float32, 16385, (2, 2, 2, 2)),
    (BF16, 9, (0, 5, 0, 0)),
    (BF16, 16384, (0, 0, 1, 3)),
]

# More tensors (one chunk each) than the finalize kernel's 1024 threads.
TINY_COUNT = 1100

# (weight_decay, grad_scale) cases of the clipped step
CLIP_CASES = [(0.0, 1.0), (0.1, -0.5)]

# Largest relative deviation of ref.multi_tensor_sumsq in fp32 from the fp64
# sum of squares of the same values, over adam_inputs()'s gradients,
# second_grads() and tiny_inputs(), measured on the CPU:
SUMSQ_D = 1.75e-07
# Largest relative deviation between the clipped ref.adamw_step run in fp32
# (with the fp32 sumsq) and in fp64 (with the fp64 one), max_grad_norm at
# half the true norm, over ADAM_STEPS and CLIP_CASES on adam_inputs(), and
# over graph_reference()'s two steps, measured on the CPU.  m and v
# are relative to the fp64 value; parameters are relative to |p| + lr, as
# the AdamW edge test explains.
CLIP_D_M, CLIP_D_V, CLIP_D_P = 2.26e-07, 3.55e-07, 4.72e-07
# The kernels are allowed 8x these, the margin for another, equally valid
# fp32 evaluation order.


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def adam_inputs():
    """CPU (dtype, p, g, offsets) per tensor, seeded: shared with the CPU
    measurement of the deviations above."""
    g = _gen(150)
    specs = [(BF16, n, (0, 0, 0, 0)) for n in ADAM_BF16_NUMELS] + \
        [(torch.float32, n, (0, 0, 0, 0)) for n in ADAM_FP32_NUMELS] + \
        ADAM_MISALIGNED
    return [(dt, torch.randn(n, generator=g).to(dt),
             torch.randn(n, generator=g).to(dt), offs)
            for dt, n, offs in specs]


def second_grads():
    """Another gradient set for adam_inputs(), three times as large."""
    g = _gen(151)
    return [(3.0 * torch.randn(p.numel(), generator=g)).to(dt)
            for dt, p, _, _ in adam_inputs()]


def tiny_inputs():
    """TINY_COUNT tensors of 1 to 5 elements, bf16 and fp32 alternating."""
    g = _gen(152)
    return [torch.randn(1 + i % 5, generator=g).to(
        BF16 if i % 2 == 0 else torch.float32) for i in range(TINY_COUNT)]


def sumsq64(tensors):
    return sum((t.double() ** 2).sum() for t in tensors)


def clipped_reference(dtype, weight_decay, grad_scale):
    """The clipped reference over ADAM_STEPS on adam_inputs() in `dtype`
    (fp32 or fp64); yields (step, p, m, v) lists after each step."""
    inputs = adam_inputs()
    up = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    p = [up(x[1].clone()) for x in inputs]
    g = [up(x[2]) for x in inputs]
    m = [torch.zeros(x[1].numel(), dtype=dtype) for x in inputs]
    v = [torch.zeros(x[1].numel(), dtype=dtype) for x in inputs]
    sumsq = ref.multi_tensor_sumsq(g)
    max_norm = clip_max_norm(grad_scale)
    for step in ADAM_STEPS:
        ref.adamw_step(p, g, m, v, step, lr=ADAM_LR, beta1=ADAM_B1,
                       beta2=ADAM_B2, eps=ADAM_EPS,
                       weight_decay=weight_decay, grad_scale=grad_scale,
                       grad_sumsq=sumsq, max_grad_norm=max_norm)
        yield step, p, m, v


def clip_max_norm(grad_scale):
    """Half the true norm of adam_inputs()'s scaled gradients."""
    return 0.5 * abs(grad_scale) * \
        sumsq64([x[2] for x in adam_inputs()]).sqrt().item()


GRAPH_STEP = 2   # the step number baked into the captured launch


def graph_reference(dtype):
    """The graph test's replays in `dtype`: from zero moments, one step on
    adam_inputs()'s gradients and one on second_grads(), both clipped at
    clip_max_norm(1.0); yields (sumsq, m, v) for each.  Starting each from
    zero keeps m = (1 - beta1) * coefficient * g free of cancellation, so
    its error relative to the result stays bounded."""
    inputs = adam_inputs()
    up = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t)
    for grads in ([x[2] for x in inputs], second_grads()):
        grads = [up(t) for t in grads]
        p = [up(x[1].clone()) for x in inputs]
        m = [torch.zeros(x[1].numel(), dtype=dtype) for x in inputs]
        v = [torch.zeros(x[1].numel(), dtype=dtype) for x in inputs]
        sumsq = ref.multi_tensor_sumsq(grads)
        ref.adamw_step(p, grads, m, v, GRAPH_STEP, lr=ADAM_LR, beta1=ADAM_B1,
                       beta2=ADAM_B2, eps=ADAM_EPS, weight_decay=0.0,
                       grad_scale=1.0, grad_sumsq=sumsq,
                       max_grad_norm=clip_max_norm(1.0))
        yield sumsq, m, v


# --------------------------------------------------------------- GPU helpers

@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _guarded(t, fill, shift):
    """A GPU buffer [guard | shift | t | guard], all but t filled with the
    sentinel; returns (buffer, view of t, offset of t)."""
    n = t.numel()
    lo = ADAM_GUARD + shift
    buf = torch.full((lo + n + ADAM_GUARD,), fill, dtype=t.dtype,
                     device="cuda")
    buf[lo:lo + n] = t.cuda()
    view = buf[lo:lo + n]
    assert (view.data_ptr() % 16 == 0) == \
        (shift * t.element_size() % 16 == 0)
    return buf, view, lo


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _guards_intact(buf, lo, fill):
    want = torch.full((buf.numel(),), fill, dtype=buf.dtype, device="cuda")
    return (torch.equal(_bits(buf[:lo]), _bits(want[:lo])) and
            torch.equal(_bits(buf[-ADAM_GUARD:]),
                        _bits(want[-ADAM_GUARD:])))


class _State:
    """adam_inputs() on the GPU behind guards, zero moments."""

    def __init__(self):
        self.bufs, self.ps, self.gs, self.ms, self.vs = [], [], [], [], []
        for dt, p, g, offs in adam_inputs():
            for src, views, shift in ((p, self.ps, offs[0]),
                                      (g, self.gs, offs[1]),
                                      (torch.zeros(p.numel()), self.ms,
                                       offs[2]),
                                      (torch.zeros(p.numel()), self.vs,
                                       offs[3])):
                buf, view, lo = _guarded(src, FILL, shift)
                self.bufs.append((buf, lo))
                views.append(view)

    def pmv(self):
        return self.ps + self.ms + self.vs

    def guards_intact(self):
        return all(_guards_intact(buf, lo, FILL) for buf, lo in self.bufs)


def _rel(got, want):
    return ((got - want).abs() / want.abs()).max().item()


def _check_sumsq(got, tensors, name):
    want = sumsq64(tensors).item()
    dev = abs(got.double().item() - want) / want
    print(f"sumsq {name}: relative deviation {dev:.3g} "
          f"(allowed {8 * SUMSQ_D:.3g})")
    # SUMSQ_D = 1.75e-07 measured -> 1.4e-06
    assert dev <= 8 * SUMSQ_D, (name, dev)


# --------------------------------------------------------------------- sumsq

def test_sumsq_mixed_list(ext):
    """Accuracy against fp64, bit-identical repeats, and nothing written:
    the gradients and the guards around every view keep their bits."""
    from alpa_amd import ops
    bufs, views = [], []
    for dt, _, g, offs in adam_inputs():
        buf, view, lo = _guarded(g, FILL, offs[1])
        bufs.append((buf, lo))
        views.append(view)
    before = [buf.clone() for buf, _ in bufs]
    got = ops.multi_tensor_sumsq(views)
    again = ops.multi_tensor_sumsq(views)
    assert got.shape == (1,) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(_bits(got), _bits(again))
    _check_sumsq(got, [x[2] for x in adam_inputs()], "mixed list")
    for (buf, lo), want in zip(bufs, before):
        assert torch.equal(_bits(buf), _bits(want)), "a gradient was written"
        assert _guards_intact(buf, lo, FILL)


def test_sumsq_more_partials_than_threads(ext):
    from alpa_amd import ops
    cpu = tiny_inputs()
    assert len(cpu) > 1024
    bufs, views = [], []
    for i, t in enumerate(cpu):
        buf, view, lo = _guarded(t, FILL, 0)
        bufs.append((buf, lo))
        views.append(view)
    got = ops.multi_tensor_sumsq(views)
    again = ops.multi_tensor_sumsq(views)
    assert torch.equal(_bits(got), _bits(again))
    _check_sumsq(got, cpu, "1100 tiny tensors")
    for (buf, lo), t in zip(bufs, cpu):
        assert torch.equal(_bits(buf[lo:lo + t.numel()]), _bits(t.cuda()))
        assert _guards_intact(buf, lo, FILL)


# ------------------------------------------------------------- clipped AdamW

@pytest.mark.parametrize("weight_decay,grad_scale", CLIP_CASES)
def test_clipped_adamw_mixed_list(ext, weight_decay, grad_scale):
    from alpa_amd import ops
    s = _State()
    max_norm = clip_max_norm(grad_scale)
    worst = {"m": 0.0, "v": 0.0, "p32": 0.0}
    for step, p64, m64, v64 in clipped_reference(torch.float64, weight_decay,
                                                 grad_scale):
        sumsq = ops.multi_tensor_sumsq(s.gs)
        ops.fused_adamw(s.ps, s.gs, s.ms, s.vs, step, lr=ADAM_LR,
                        beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
                        weight_decay=weight_decay, grad_scale=grad_scale,
                        grad_sumsq=sumsq, max_grad_norm=max_norm)
        for i, p in enumerate(s.ps):
            got_m, got_v = s.ms[i].double().cpu(), s.vs[i].double().cpu()
            got_p = p.double().cpu()
            worst["m"] = max(worst["m"], _rel(got_m, m64[i]))
            worst["v"] = max(worst["v"], _rel(got_v, v64[i]))
            if p.dtype != BF16:
                worst["p32"] = max(worst["p32"],
                                   ((got_p - p64[i]).abs() /
                                    (p64[i].abs() + ADAM_LR)).max().item())
        print(f"clipped adamw step {step}: worst relative deviation", worst)
        for i, p in enumerate(s.ps):
            got_m, got_v = s.ms[i].double().cpu(), s.vs[i].double().cpu()
            got_p = p.double().cpu()
            # CLIP_D_M = 2.26e-07 measured -> rtol 1.8e-06
            torch.testing.assert_close(got_m, m64[i], rtol=8 * CLIP_D_M,
                                       atol=0)
            # CLIP_D_V = 3.55e-07 measured -> rtol 2.8e-06
            torch.testing.assert_close(got_v, v64[i], rtol=8 * CLIP_D_V,
                                       atol=0)
            if p.dtype == BF16:
                # the kernel rounds the parameter to bf16 every step
                torch.testing.assert_close(got_p, p64[i], rtol=2e-2,
                                           atol=2e-2)
            else:
                # CLIP_D_P = 4.72e-07 measured -> 3.8e-06 * (|p| + lr)
                torch.testing.assert_close(got_p, p64[i], rtol=8 * CLIP_D_P,
                                           atol=8 * CLIP_D_P * ADAM_LR)
    assert s.guards_intact(), "write outside a tensor"


def test_no_clip_is_bit_identical(ext):
    """max_grad_norm far above the norm: max_norm / max(norm, max_norm) is
    exactly 1, so the effective scale is exactly grad_scale."""
    from alpa_amd import ops
    a, b = _State(), _State()
    max_norm = 2e6 * clip_max_norm(0.5)
    for step in (1, 2):
        kw = dict(lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
                  weight_decay=0.1, grad_scale=0.5)
        ops.fused_adamw(a.ps, a.gs, a.ms, a.vs, step, **kw)
        ops.fused_adamw(b.ps, b.gs, b.ms, b.vs, step, **kw,
                        grad_sumsq=ops.multi_tensor_sumsq(b.gs),
                        max_grad_norm=max_norm)
        for x, y in zip(a.pmv(), b.pmv()):
            assert torch.equal(_bits(x), _bits(y))
    assert b.guards_intact()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_is_a_noop(ext, bad):
    """The bad value sits in the last element of a scalar tail: numel 16385
    is one full vector chunk plus a one-element tail in the second chunk."""
    from alpa_amd import ops
    s = _State()
    idx = next(i for i, x in enumerate(adam_inputs())
               if x[0] == BF16 and x[1].numel() == 16385 and
               x[3] == (0, 0, 0, 0))
    kw = dict(lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
              weight_decay=0.1, grad_scale=0.5)
    # one ordinary step first, so the moments are not zero
    ops.fused_adamw(s.ps, s.gs, s.ms, s.vs, 1, **kw)
    s.gs[idx][-1] = bad
    before = [t.clone() for t in s.pmv()]
    sumsq = ops.multi_tensor_sumsq(s.gs)
    assert not torch.isfinite(sumsq).item()
    ops.fused_adamw(s.ps, s.gs, s.ms, s.vs, 2, **kw, grad_sumsq=sumsq,
                    max_grad_norm=1.0)
    for got, want in zip(s.pmv(), before):
        assert torch.equal(_bits(got), _bits(want))
    assert s.guards_intact()


def test_binding_checks_grad_sumsq(ext):
    from alpa_amd import ops
    s = _State()
    args = (s.ps, s.gs, s.ms, s.vs, 1, ADAM_LR)
    for bad in (torch.ones(1), torch.ones(2, device="cuda"),
                torch.ones(1, device="cuda", dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="grad_sumsq"):
            ops.fused_adamw(*args, grad_sumsq=bad, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        ops.fused_adamw(*args, max_grad_norm=1.0)


# ------------------------------------------------------------- graph capture

def test_sumsq_and_clipped_adamw_in_one_graph(ext):
    """sumsq and the clip coefficient never leave the device: one captured
    chain replays with each gradient set's own norm."""
    from alpa_amd import ops
    s = _State()
    max_norm = clip_max_norm(1.0)
    first = [x[2] for x in adam_inputs()]

    def run():
        sumsq = ops.multi_tensor_sumsq(s.gs)
        ops.fused_adamw(s.ps, s.gs, s.ms, s.vs, GRAPH_STEP, lr=ADAM_LR,
                        beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
                        weight_decay=0.0, grad_scale=1.0, grad_sumsq=sumsq,
                        max_grad_norm=max_norm)
        return sumsq

    reference = graph_reference(torch.float64)
    run()                                   # eager: builds the tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_sumsq = run()
    for name, grads in (("first", first), ("second", second_grads())):
        for dst, src in zip(s.gs, grads):
            dst.copy_(src)
        for t in s.ms + s.vs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        sumsq64_, m64, v64 = next(reference)
        _check_sumsq(static_sumsq, grads, f"graph replay, {name} set")
        torch.testing.assert_close(static_sumsq.double().cpu(), sumsq64_,
                                   rtol=8 * SUMSQ_D, atol=0)
        for i in range(len(s.ps)):
            torch.testing.assert_close(s.ms[i].double().cpu(), m64[i],
                                       rtol=8 * CLIP_D_M, atol=0)
            torch.testing.assert_close(s.vs[i].double().cpu(), v64[i],
                                       rtol=8 * CLIP_D_V, atol=0)
    assert s.guards_intact()


# ------------------------------------------------------------- whole model

def test_train_state_clips_tiny_gpt():
    """TrainState.create(max_grad_norm=...) on a tiny bf16 GPT: the norm the
    step reports is that of the gradients it applied, and every step clips.
    The norm's relative error is half that of sumsq plus an ulp each for the
    sqrt and the scale, so 8 * SUMSQ_D covers it."""
    import alpa_amd as aa
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    aa.init()
    cfg = GPTConfig(hidden_size=256, num_layers=2, num_heads=4, seq_len=128,
                    vocab_size=1024)
    method = aa.ShardParallel(num_micro_batches=2, logical_mesh_shape=(1, 1))

    def build(mesh=None, axis=1, dtype=BF16, device=None):
        torch.manual_seed(0)
        return GPTModel(cfg, mesh, axis, dtype, device)

    max_norm = 0.05
    state = aa.TrainState.create(build, method, lr=1e-3,
                                 max_grad_norm=max_norm)
    step = aa.parallelize(lambda m, b: m.loss(b[0], b[1]), method=method)
    g = _gen(7)
    ids = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len),
                        generator=g).cuda()
    labels = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len),
                           generator=g).cuda()
    losses = []
    for _ in range(3):
        losses.append(float(step(state, (ids, labels))))
        # the summed microbatch gradients are still in place after the
        # step; it applied them times 1 / num_micro_batches
        want = 0.5 * sumsq64([p.grad for p in state.model.parameters()
                              if p.grad is not None]).sqrt().item()
        got = state.optimizer.last_grad_norm
        assert got.is_cuda and got.numel() == 1
        print(f"tiny GPT grad norm {got.item():.6g} (fp64 {want:.6g})")
        assert want > max_norm, "the step was not clipped"
        assert abs(got.item() - want) <= 8 * SUMSQ_D * want
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
