"""Softmax-cross-entropy over vocab shards, CPU side: the reference
partial / combine / shard-backward functions against the full-vocab
reference in fp64, the one-collective autograd function over gloo, and the
default routing of CPU tensors.
"""
import pytest
import torch
import torch.nn.functional as F

from dist_utils import run_distributed

import alpa_amd as aa
from alpa_amd import ops
from alpa_amd.ops import reference as ref
from alpa_amd.parallel import layers

NEG = float("-inf")
VS = 16                      # equal split: three shards of VS columns
NO_OWNER = 7                 # the row whose target no shard owns


def _hostile(widths):
    """fp64 logits [8, 3*VS] and targets for a split into `widths`:
    rows 0-5 have their targets on the first and last column of every
    shard, row 6 is -inf all over the middle shard, row 7's target is past
    the vocab."""
    V = sum(widths)
    starts = [0, widths[0], widths[0] + widths[1]]
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(8, V, generator=g, dtype=torch.float64) * 3
    edges = [c for s, w in zip(starts, widths) for c in (s, s + w - 1)]
    logits[6, starts[1]:starts[2]] = NEG
    targets = torch.tensor(edges + [starts[2] + 1, V], dtype=torch.int64)
    dloss = torch.randn(8, generator=g, dtype=torch.float64)
    return logits, targets, dloss, starts


@pytest.mark.parametrize("widths", [(VS, VS, VS), (8, 24, 16)])
def test_shards_match_full_vocab_reference(widths):
    assert sum(widths) == 3 * VS
    logits, targets, dloss, starts = _hostile(widths)
    shards = [logits[:, s:s + w].contiguous()
              for s, w in zip(starts, widths)]
    stats = torch.stack([ref.softmax_cross_entropy_partial(x, targets, s)
                         for x, s in zip(shards, starts)])
    assert stats.dtype == torch.float64 and stats.shape == (3, 3, 8)
    assert not torch.isnan(stats).any()

    # ownership: exactly one shard carries each owned target, bit for bit
    t = stats[:, 2]
    for row in range(8):
        tgt = targets[row].item()
        for r, (s, w) in enumerate(zip(starts, widths)):
            want = logits[row, tgt].item() if s <= tgt < s + w else 0.0
            assert t[r, row].item() == want, (row, r)
    assert (t[:, NO_OWNER] == 0).all()
    # the fully masked shard row
    assert stats[1, 0, 6].item() == NEG and stats[1, 1, 6].item() == 0.0

    loss, lse = ops.softmax_cross_entropy_combine(stats)
    # the full-vocab reference cannot index row 7's target: give it column
    # 0 there and take the one-hot back out by hand
    safe = targets.clone()
    safe[NO_OWNER] = 0
    loss64, lse64 = ref.softmax_cross_entropy_fwd(logits, safe)
    loss64[NO_OWNER] = lse64[NO_OWNER]
    torch.testing.assert_close(lse, lse64, rtol=1e-12, atol=0)
    torch.testing.assert_close(loss, loss64, rtol=1e-12, atol=1e-12)

    d64 = ref.softmax_cross_entropy_bwd(dloss, logits, safe, lse64)
    d64[NO_OWNER, 0] += dloss[NO_OWNER]
    got = torch.cat([ref.softmax_cross_entropy_shard_bwd(dloss, x, targets,
                                                         lse64, s)
                     for x, s in zip(shards, starts)], dim=-1)
    torch.testing.assert_close(got, d64, rtol=1e-12, atol=1e-12)
    assert (got[6, starts[1]:starts[2]] == 0).all()


def test_ops_dispatch_cpu_tensors_to_reference():
    logits, targets, dloss, _ = _hostile((VS, VS, VS))
    x = logits[:, :VS].contiguous()
    stats = ops.softmax_cross_entropy_partial(x, targets, 0)
    assert torch.equal(stats, ref.softmax_cross_entropy_partial(x, targets, 0))
    lse = stats[0] + torch.log(stats[1])
    assert torch.equal(
        ops.softmax_cross_entropy_shard_bwd(dloss, x, targets, lse, 0),
        ref.softmax_cross_entropy_shard_bwd(dloss, x, targets, lse, 0))
    # half precision computes in fp32
    assert ops.softmax_cross_entropy_partial(
        x.to(torch.bfloat16), targets, 0).dtype == torch.float32
    assert not ops.vocab_ce_fused_ok(x.to(torch.bfloat16))


def test_fused_function_single_process_matches_full_vocab():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(10, 24, generator=g).requires_grad_()
    targets = torch.randint(0, 24, (10,), generator=g)
    w = torch.randn(10, generator=g)
    loss = layers.fused_vocab_parallel_cross_entropy(logits, targets, None,
                                                     1, 0)
    (loss * w).sum().backward()
    ref_logits = logits.detach().clone().requires_grad_()
    want = F.cross_entropy(ref_logits, targets, reduction="none")
    (want * w).sum().backward()
    torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(logits.grad, ref_logits.grad, rtol=1e-5,
                               atol=1e-5)


GLOO_N, GLOO_VS = 12, 10


def _gloo_inputs(world_size):
    g = torch.Generator().manual_seed(11)
    full = torch.randn(GLOO_N, world_size * GLOO_VS, generator=g) * 3
    targets = torch.randint(0, world_size * GLOO_VS, (GLOO_N,), generator=g)
    # both ends of the vocab and a shard boundary
    targets[0], targets[1] = 0, world_size * GLOO_VS - 1
    targets[2], targets[3] = GLOO_VS - 1, GLOO_VS
    w = torch.randn(GLOO_N, generator=g)
    return full, targets, w


def _fused_worker(rank, world_size):
    mesh = aa.full_mesh((1, world_size))
    full, targets, w = _gloo_inputs(world_size)
    start = mesh.axis_index(1) * GLOO_VS
    local = full[:, start:start + GLOO_VS].clone().requires_grad_()
    loss = layers.fused_vocab_parallel_cross_entropy(local, targets, mesh, 1,
                                                     start)
    (loss * w).sum().backward()
    return {"loss": loss.detach(), "grad": local.grad}


@pytest.mark.parametrize("world_size", [2, 4])
def test_fused_vocab_parallel_cross_entropy_gloo(world_size):
    res = run_distributed(_fused_worker, world_size=world_size)
    full, targets, w = _gloo_inputs(world_size)
    full.requires_grad_()
    want = F.cross_entropy(full, targets, reduction="none")
    (want * w).sum().backward()
    # fp32 exp/log at |lse| ~ 10
    torch.testing.assert_close(res[0]["loss"], want.detach(), rtol=1e-5,
                               atol=1e-5)
    grad = torch.cat([r["grad"] for r in res], dim=-1)
    torch.testing.assert_close(grad, full.grad, rtol=1e-5, atol=1e-5)
    for r in res[1:]:
        assert torch.equal(r["loss"], res[0]["loss"]), "ranks disagree"


@pytest.mark.parametrize("dtype,width", [(torch.float32, 24),
                                         (torch.bfloat16, 24),
                                         (torch.float32, 10)])
def test_default_routing_keeps_cpu_on_the_torch_path(dtype, width):
    """A tp = 2 mesh in a single process: the collectives are no-ops, so
    the loss is that of shard 0 alone; what matters is which function ran."""
    mesh = aa.DeviceMesh([0, 1], (1, 2))
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(6, width, generator=g).to(dtype).requires_grad_()
    targets = torch.randint(0, width, (6,), generator=g)
    loss = layers.vocab_parallel_cross_entropy(logits, targets, mesh, 1, 0)
    assert type(loss.grad_fn).__name__ == "_VocabParallelCrossEntropyBackward"
    fused = layers.fused_vocab_parallel_cross_entropy(logits, targets, None,
                                                      1, 0)
    assert type(fused.grad_fn).__name__ == \
        "_FusedVocabParallelCrossEntropyBackward"
