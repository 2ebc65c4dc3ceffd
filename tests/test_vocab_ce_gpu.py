"""The vocab-shard softmax-cross-entropy kernels on one GPU.

Three tensor-parallel shards are emulated by slicing a [8, 3*Vs] bf16
tensor into contiguous copies; each goes through the partial-forward and
shard-backward kernels with its own vocab_start, and the combine runs on
the stacked statistics.  The oracle is alpa_amd.ops.reference on fp64
copies of the bf16 inputs, over the whole vocab.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd import ops
from alpa_amd.ops import reference as ref

BF16 = torch.bfloat16
NEG = float("-inf")
T = 3

# shard widths: one thread does all the work / some threads idle / thread 0
# takes a second trip and the last trip is partial / the tp = 8 model shard
WIDTHS = [8, 1000, 2056, 6400]


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(Vs):
    """logits bf16 [8, 3*Vs] and targets int64 [8], on the CPU."""
    V = T * Vs
    logits = torch.randn(8, V, generator=_gen(150))
    tgt = [0] * 8
    tgt[0] = 0                               # unit normals, column 0
    logits[1] = 2.5                          # all equal: each carries 1/V of s
    tgt[1] = Vs + 3
    spike = Vs - 1                           # last column of shard 0
    logits[2] = -3e4                         # spike, target on it
    logits[2, spike] = 3e4
    tgt[2] = spike
    logits[3] = -3e4                         # spike, target on another shard
    logits[3, spike] = 3e4
    tgt[3] = 2 * Vs
    logits[4, Vs:2 * Vs] = NEG               # shard 1 fully masked,
    logits[4, :2] = NEG                      # shard 0 masked at both ends
    logits[4, Vs - 2:Vs] = NEG
    tgt[4] = 2 * Vs + 5
    logits[5] *= 50.0                        # large magnitudes
    tgt[5] = V - 1
    tgt[6] = Vs - 1                          # ownership at the boundary
    tgt[7] = Vs
    return logits.to(BF16), torch.tensor(tgt, dtype=torch.int64)


def _shards(logits, Vs):
    return [logits[:, r * Vs:(r + 1) * Vs].contiguous() for r in range(T)]


@pytest.mark.parametrize("Vs", WIDTHS)
def test_partial_stats_and_combine(ext, Vs):
    cpu_logits, cpu_targets = _rows(Vs)
    logits, targets = cpu_logits.cuda(), cpu_targets.cuda()
    l64 = logits.double()
    assert l64[4, cpu_targets[4]].item() != NEG
    stats = torch.stack([ext.cross_entropy_partial_fwd(x, targets, r * Vs)
                         for r, x in enumerate(_shards(logits, Vs))])
    assert stats.shape == (T, 3, 8) and stats.dtype == torch.float32
    assert not torch.isnan(stats).any()

    worst = 0.0
    for r in range(T):
        x64 = l64[:, r * Vs:(r + 1) * Vs]
        m, s, t = stats[r].double()
        # maxima of bf16 values are exact
        m64 = x64.max(-1).values
        assert torch.equal(m, m64), (r, m.tolist(), m64.tolist())
        # the target logit is copied, not computed
        local = targets - r * Vs
        owned = (local >= 0) & (local < Vs)
        t64 = torch.where(
            owned, x64.gather(-1, local.clamp(0, Vs - 1)[:, None])[:, 0],
            torch.zeros_like(m64))
        assert torch.equal(t, t64), (r, t.tolist(), t64.tolist())
        # s within rtol 5e-5.  Derived, not measured: the terms that matter
        # have |x - m| <= 20, where __expf is off by at most ~1.3e-6
        # relative; an fp32 sum of positive terms at depth <= 40 (25 adds
        # per thread at Vs = 6400, 6 + 2 reduction levels, the rescales)
        # adds at most 2.4e-6.  Together ~4e-6, a margin of ~10x.  One lost
        # element of row 1 at Vs = 6400 moves s by 1.6e-4.
        finite = ~torch.isinf(m64)
        shift = torch.where(finite, m64, torch.zeros_like(m64))
        s64 = torch.exp(x64 - shift[:, None]).sum(-1)
        # where s64 = 0 (the fully masked shard row) only s = 0 passes
        err = (s - s64).abs() / (5e-5 * s64).clamp_min(1e-300)
        worst = max(worst, err.max().item())
    print(f"Vs={Vs}: s worst err/bound = {worst:.3g}")
    assert worst <= 1.0, worst

    # row 4, shard 1: nothing finite
    assert stats[1, 0, 4].item() == NEG
    assert stats[1, 1, 4].item() == 0.0 and stats[1, 2, 4].item() == 0.0

    loss, lse = ops.softmax_cross_entropy_combine(stats)
    loss64, lse64 = ref.softmax_cross_entropy_fwd(l64, targets)
    print("lse got", lse.tolist(), "want", lse64.tolist())
    torch.testing.assert_close(lse.double(), lse64, rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(loss.double(), loss64, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("Vs", WIDTHS)
def test_targets_no_shard_owns(ext, Vs):
    """Negative ids and ids past the vocab belong to no shard: t is 0 on
    every shard and the rest of the statistics are those of valid targets.
    Values only: the kernel decides ownership before it forms an address."""
    cpu_logits, cpu_targets = _rows(Vs)
    logits, targets = cpu_logits[:3].cuda(), cpu_targets[:3].cuda()
    outside = torch.tensor([-1, T * Vs, 2 ** 40], dtype=torch.int64).cuda()
    for r, x in enumerate(_shards(logits, Vs)):
        got = ext.cross_entropy_partial_fwd(x, outside, r * Vs)
        want = ext.cross_entropy_partial_fwd(x, targets, r * Vs)
        assert (got[2] == 0).all(), (r, got[2].tolist())
        assert torch.equal(got[:2], want[:2])


@pytest.mark.parametrize("Vs", WIDTHS)
def test_shard_backward(ext, Vs):
    V = T * Vs
    cpu_logits, cpu_targets = _rows(Vs)
    logits, targets = cpu_logits.cuda(), cpu_targets.cuda()
    l64 = logits.double()
    _, lse64 = ref.softmax_cross_entropy_fwd(l64, targets)
    lse32 = lse64.float()
    dloss = torch.randn(8, generator=_gen(151)).cuda()
    dlogits = torch.cat(
        [ext.cross_entropy_shard_bwd(dloss, x, targets, lse32, r * Vs)
         for r, x in enumerate(_shards(logits, Vs))], dim=-1)
    d64 = ref.softmax_cross_entropy_bwd(dloss.double(), l64, targets,
                                        lse32.double())
    assert dlogits.dtype == BF16 and torch.isfinite(dlogits).all()
    torch.testing.assert_close(dlogits.double(), d64, rtol=2e-2, atol=2e-2)
    # softmax - onehot sums to zero; what is left is bf16 output rounding
    rowsum = dlogits.double().sum(-1).abs()
    bound = 2.0 ** -8 * dloss.double().abs() * math.sqrt(V)
    assert (rowsum <= bound).all(), (rowsum.tolist(), bound.tolist())
    masked = logits[4] == NEG
    assert masked.sum().item() == Vs + 4
    assert (dlogits[4][masked] == 0).all()
    # row 3: the one-hot comes off once, on the owner (shard 2), and the
    # spike on shard 0 keeps its whole softmax weight of 1
    dl = dloss[3].double().item()
    tol = 2e-2 * abs(dl) + 1e-6
    assert abs(dlogits[3, 2 * Vs].double().item() + dl) <= tol
    assert abs(dlogits[3, Vs - 1].double().item() - dl) <= tol


@pytest.mark.parametrize("V", [2056, 51200])
def test_shard_backward_is_the_full_backward_at_start_zero(ext, V):
    g = _gen(152)
    logits = (torch.randn(4, V, generator=g) * 3).to(BF16).cuda()
    targets = torch.tensor([0, 7, V // 2 + 1, V - 1]).cuda()
    dloss = torch.randn(4, generator=g).cuda()
    _, lse = ext.cross_entropy_fwd(logits, targets)
    want = ext.cross_entropy_bwd(dloss, logits, targets, lse)
    got = ext.cross_entropy_shard_bwd(dloss, logits, targets, lse, 0)
    assert torch.equal(got, want)


def test_bindings_reject_what_the_kernels_cannot_read(ext):
    logits = torch.zeros(4, 24, dtype=BF16).cuda()
    targets = torch.zeros(4, dtype=torch.int64).cuda()
    lse = torch.zeros(4).cuda()
    dloss = torch.ones(4).cuda()
    bad = [
        (logits.float(), targets),                   # not bf16
        (logits[:, :16], targets),                   # not contiguous
        (logits[:, :12].contiguous(), targets),      # width % 8 != 0
        (logits.view(-1)[4:4 + 32].view(2, 16), targets[:2]),  # 8-byte aligned
        (logits, targets.int()),                     # int32 targets
        (logits, targets[:3]),                       # one target short
    ]
    for x, tg in bad:
        with pytest.raises(RuntimeError):
            ext.cross_entropy_partial_fwd(x, tg, 0)
        with pytest.raises(RuntimeError):
            ext.cross_entropy_shard_bwd(dloss[:x.shape[0]], x, tg,
                                        lse[:x.shape[0]], 0)
    with pytest.raises(RuntimeError):
        ext.cross_entropy_partial_fwd(logits, targets, -8)
    assert ops.vocab_ce_fused_ok(logits)
    for x, _ in bad[:4]:
        assert not ops.vocab_ce_fused_ok(x)


def test_autograd_glue_and_graph_capture():
    import alpa_amd as aa
    from alpa_amd.parallel.layers import fused_vocab_parallel_cross_entropy
    mesh = aa.DeviceMesh([0], (1, 1))
    g = _gen(154)
    N, V = 16, 1000
    data = torch.randn(N, V, generator=g).to(BF16).cuda()
    targets = torch.randint(0, V, (N,), generator=g).cuda()

    def run(fn, x):
        x.grad = None
        loss = fn(x)
        loss.mean().backward()
        return loss.detach(), x.grad

    x = data.clone().requires_grad_()
    loss, grad = run(lambda x: fused_vocab_parallel_cross_entropy(
        x, targets, mesh, 1, 0), x)
    y = data.clone().requires_grad_()
    loss_ref, grad_ref = run(lambda y: ops.softmax_cross_entropy(y, targets),
                             y)
    torch.testing.assert_close(loss, loss_ref, rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(grad.float(), grad_ref.float(), rtol=2e-2,
                               atol=2e-2)

    # no host sync anywhere: the same step captures and replays
    static = data.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(lambda s: fused_vocab_parallel_cross_entropy(
            s, targets, mesh, 1, 0), static)
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss = fused_vocab_parallel_cross_entropy(static, targets, mesh, 1,
                                                    0)
        g_loss.mean().backward()
    g_grad = static.grad
    g_loss.detach().zero_()
    g_grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_loss.detach(), loss)
    assert torch.equal(g_grad, grad)
