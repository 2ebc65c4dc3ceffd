"""Global-norm gradient clipping on the CPU path: the pure-torch reference
against torch.nn.utils.clip_grad_norm_, the no-op on a non-finite gradient,
argument checking, and TrainState.create(max_grad_norm=...) under dp,
ZeRO-2, ZeRO-3 and dp with expert parallelism against the serial run (gloo,
world_size=2)."""
import functools

import pytest
import torch
import torch.nn as nn

from dist_utils import run_distributed

import alpa_amd as aa
from alpa_amd import ops
from alpa_amd.models.moe import MoEConfig, MoEGPTModel
from alpa_amd.ops import reference as ref
from alpa_amd.optim import AdamW
from alpa_amd.parallel.layers import ColumnParallelLinear, RowParallelLinear

LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.95, 1e-8, 0.1
SHAPES = [(1,), (7,), (33, 5), (16385,)]


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in SHAPES]


def _true_norm(grads, grad_scale):
    return abs(grad_scale) * torch.sqrt(
        sum((t.double() ** 2).sum() for t in grads)).item()


# ------------------------------------------------- agreement with torch

# torch's coefficient is max_norm / (norm + 1e-6) against optax's
# max_norm / norm: with norm between 32 and 128 here they differ by at most
# 3e-8 relative, below fp32 rounding.  What is left is fp32 rounding of
# sumsq (16k terms), the coefficient and one extra multiply per gradient, a
# few ulp each; v carries the coefficient squared.  1e-5 is ~80 ulp, and a coefficient that is
# missing, applied twice or not squared in v is off by 0.5 or more.
RTOL = 1e-5


@pytest.mark.parametrize("grad_scale", [1.0, -0.25])
@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_clipped_reference_matches_clip_grad_norm(factor, grad_scale):
    """max_grad_norm at factor x the true norm: below it (coefficient 0.5)
    and above it (coefficient 1).  Adam's parameter update is nearly
    invariant to a uniform gradient scale, so the moments carry the check:
    exp_avg scales by the coefficient and exp_avg_sq by its square."""
    p0, grads = _tensors(1), _tensors(2)
    norm = _true_norm(grads, grad_scale)
    max_norm = factor * norm
    coef = min(1.0, factor)

    # what a user does without the feature: scale, clip in place, step
    holders = [nn.Parameter(p.clone()) for p in p0]
    for h, g in zip(holders, grads):
        h.grad = g.clone() * grad_scale
    torch_norm = torch.nn.utils.clip_grad_norm_(holders, max_norm)
    want_p = [p.clone() for p in p0]
    want_m = [torch.zeros_like(p) for p in p0]
    want_v = [torch.zeros_like(p) for p in p0]
    plain_m = [torch.zeros_like(p) for p in p0]
    plain_v = [torch.zeros_like(p) for p in p0]

    params = [nn.Parameter(p.clone()) for p in p0]
    opt = AdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD,
                max_grad_norm=max_norm)
    for step in (1, 2):
        ref.adamw_step(want_p, [h.grad for h in holders], want_m, want_v,
                       step, LR, B1, B2, EPS, WD)
        ref.adamw_step([p.clone() for p in p0], grads, plain_m, plain_v,
                       step, LR, B1, B2, EPS, 0.0, grad_scale)
        opt.step(grads=grads, grad_scale=grad_scale)
        torch.testing.assert_close(opt.last_grad_norm.reshape(()),
                                   torch_norm.reshape(()), rtol=RTOL, atol=0)
        torch.testing.assert_close(opt.last_grad_norm.item(), norm,
                                   rtol=RTOL, atol=0)
        for i in range(len(p0)):
            torch.testing.assert_close(opt.exp_avgs[i], want_m[i],
                                       rtol=RTOL, atol=0)
            torch.testing.assert_close(opt.exp_avg_sqs[i], want_v[i],
                                       rtol=RTOL, atol=0)
            # relative to the unclipped moments: the coefficient itself
            torch.testing.assert_close(opt.exp_avgs[i], coef * plain_m[i],
                                       rtol=RTOL, atol=0)
            torch.testing.assert_close(opt.exp_avg_sqs[i],
                                       coef * coef * plain_v[i],
                                       rtol=RTOL, atol=0)
            torch.testing.assert_close(params[i].data, want_p[i],
                                       rtol=1e-4, atol=1e-6)


def test_sumsq_reference_mixed_dtypes():
    ts = _tensors(3)
    ts[1] = ts[1].to(torch.bfloat16)
    ts[3] = ts[3].to(torch.bfloat16)[3:]     # a view at an odd offset
    got = ops.multi_tensor_sumsq(ts)
    assert got.shape == (1,) and got.dtype == torch.float32
    want = sum((t.double() ** 2).sum() for t in ts)
    torch.testing.assert_close(got.double().reshape(()), want, rtol=1e-6,
                               atol=0)
    assert torch.equal(got, ref.multi_tensor_sumsq(ts))


# ------------------------------------------------- non-finite gradient

@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_is_a_noop(bad):
    p, grads = _tensors(4), _tensors(5)
    m = [torch.rand_like(t) for t in p]
    v = [torch.rand_like(t) for t in p]
    grads[2][17, 3] = bad
    before = [t.clone() for t in p + m + v]
    sumsq = ops.multi_tensor_sumsq(grads)
    assert not torch.isfinite(sumsq).item()
    ops.fused_adamw(p, grads, m, v, 3, LR, B1, B2, EPS, WD, 0.5,
                    grad_sumsq=sumsq, max_grad_norm=1.0)
    for got, want in zip(p + m + v, before):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------- argument errors

def test_argument_errors():
    p, g = _tensors(6), _tensors(7)
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    sumsq = ops.multi_tensor_sumsq(g)
    for fn in (ops.fused_adamw, ref.adamw_step):
        args = (p, g, m, v, 1, LR, B1, B2, EPS, 0.0, 1.0)
        with pytest.raises(ValueError):
            fn(*args, grad_sumsq=sumsq)
        with pytest.raises(ValueError):
            fn(*args, max_grad_norm=1.0)
        with pytest.raises(ValueError):
            fn(*args, grad_sumsq=sumsq, max_grad_norm=0.0)
        with pytest.raises(ValueError):
            fn(*args, grad_sumsq=sumsq, max_grad_norm=-1.0)
    with pytest.raises(ValueError):
        AdamW([nn.Parameter(p[0])], max_grad_norm=0.0)
    # nothing above touched the state
    assert all(not t.any() for t in m + v)


# ------------------------------------- TrainState against the serial run

HIDDEN = 256
BATCH = 8
STEPS = 3
NMB = 2
# The serial run's gradient norms are 1.10, 1.02 and 1.02 (asserted to exceed
# this in test_serial_run_is_clipped), so every step is clipped.
MAX_GRAD_NORM = 0.5


def build_mlp(mesh=None, axis=1, dtype=torch.float32, device=None):
    torch.manual_seed(42)

    class MLP(nn.Module):

        def __init__(self):
            super().__init__()
            self.l1 = ColumnParallelLinear(HIDDEN, 4 * HIDDEN, mesh, axis,
                                           gelu=True, dtype=dtype,
                                           device=device)
            self.l2 = RowParallelLinear(4 * HIDDEN, HIDDEN, mesh, axis,
                                        dtype=dtype, device=device)
            self.l3 = ColumnParallelLinear(HIDDEN, 4 * HIDDEN, mesh, axis,
                                           gelu=True, dtype=dtype,
                                           device=device)
            self.l4 = RowParallelLinear(4 * HIDDEN, HIDDEN, mesh, axis,
                                        dtype=dtype, device=device)
            # a parameter outside every child module, like GPT's wpe: under
            # ZeRO-3 it stays replicated, so the composite optimizer has to
            # add its squares to the shards' for the one global norm
            self.gain = nn.Parameter(torch.ones(HIDDEN, dtype=dtype,
                                                device=device))

        def forward(self, x):
            return self.l4(self.l3(self.l2(self.l1(x * self.gain))))

    return MLP()


def loss_fn(model, batch):
    x, y = batch
    return ((model(x) - y) ** 2).mean()


def make_batch(step: int):
    g = torch.Generator().manual_seed(1000 + step)
    x = torch.randn(BATCH, HIDDEN, generator=g)
    y = torch.randn(BATCH, HIDDEN, generator=g)
    return x, y


def _train(method, dp, collect_params):
    """STEPS clipped steps; returns (per-step last_grad_norm, params)."""
    state = aa.TrainState.create(build_mlp, method, lr=1e-3,
                                 max_grad_norm=MAX_GRAD_NORM)
    step = aa.parallelize(loss_fn, method=method)
    idx = state.mesh.axis_index(0) if dp > 1 else 0
    per = BATCH // dp
    norms = []
    for i in range(STEPS):
        x, y = make_batch(i)
        step(state, (x[idx * per:(idx + 1) * per],
                     y[idx * per:(idx + 1) * per]))
        norm = state.optimizer.last_grad_norm
        assert torch.is_tensor(norm) and norm.numel() == 1
        norms.append(norm.reshape(()).clone())
    return torch.stack(norms), collect_params(state)


def _model_params(state):
    return [p.detach().clone() for p in state.model.parameters()]


def _zero3_params(state):
    # model.parameters() order: the module's own parameter (gain, the
    # replicated rest under ZeRO-3) first, then the children's
    rest = state.optimizer.rest_opt
    assert rest is not None and len(rest.params) == 1
    params = [p.detach().clone() for p in rest.params]
    for b in state.zero3_manager.blocks:
        b.gather(state.zero3_manager.group)
        params.extend(p.detach().clone() for p in b.params)
        b.release()
    return params


@functools.lru_cache(maxsize=None)
def serial_run():
    method = aa.ShardParallel(num_micro_batches=NMB,
                              logical_mesh_shape=(1, 1))
    return _train(method, 1, _model_params)


def _worker(rank, world_size, kind):
    if kind == "dp":
        method = aa.ShardParallel(num_micro_batches=NMB,
                                  logical_mesh_shape=(2, 1))
        return _train(method, 2, _model_params)
    if kind == "zero2":
        return _train(aa.Zero2Parallel(num_micro_batches=NMB), 2,
                      _model_params)
    if kind == "zero3":
        return _train(aa.Zero3Parallel(num_micro_batches=NMB), 2,
                      _zero3_params)
    if kind == "ep":
        return _train_moe(aa.ShardParallel(logical_mesh_shape=(2, 1)), 2)
    build, method = {
        "tp": (build_mlp, aa.ShardParallel(logical_mesh_shape=(1, 2))),
        "ep_zero2": (build_moe, aa.Zero2Parallel()),
        "ep_zero3": (build_moe, aa.Zero3Parallel()),
    }[kind]
    try:
        aa.TrainState.create(build, method, lr=1e-3,
                             max_grad_norm=MAX_GRAD_NORM)
    except NotImplementedError as e:
        return str(e)
    return ""


def test_serial_run_is_clipped():
    """The coefficient is below 1 at every step of the serial run."""
    norms, _ = serial_run()
    assert (norms > MAX_GRAD_NORM).all(), norms
    print("serial grad norms", norms.tolist())


@pytest.mark.parametrize("kind", ["dp", "zero2", "zero3"])
def test_clipped_parallel_matches_serial(kind):
    serial_norms, serial_params = serial_run()
    results = run_distributed(_worker, world_size=2, args=(kind,))
    for rank_norms, rank_params in results:
        # the norm is a sum over 1.3M gradients regrouped by rank and
        # bucket: fp32 rounding only
        torch.testing.assert_close(rank_norms, serial_norms, rtol=1e-5,
                                   atol=0)
        assert len(rank_params) == len(serial_params)
        for sp, rp in zip(serial_params, rank_params):
            torch.testing.assert_close(rp, sp, rtol=1e-4, atol=1e-5)


def test_tp2_raises():
    for msg in run_distributed(_worker, world_size=2, args=("tp",)):
        assert "tp > 1" in msg, msg


@pytest.mark.parametrize("kind", ["ep_zero2", "ep_zero3"])
def test_expert_parallel_under_zero_raises(kind):
    for msg in run_distributed(_worker, world_size=2, args=(kind,)):
        assert "expert parallelism" in msg, msg


def test_pipeline_raises():
    with pytest.raises(NotImplementedError, match="PipeshardParallel"):
        aa.TrainState.create(None, aa.PipeshardParallel(num_stages=2),
                             max_grad_norm=1.0)


# ------------------------------------------- expert parallelism over dp

MOE_CFG = MoEConfig(hidden_size=64, num_layers=2, num_heads=4, seq_len=16,
                    vocab_size=96, num_experts=4, moe_every=2,
                    capacity_factor=8.0, aux_loss_weight=0.0)
MOE_STEPS = 2
# The serial MoE run's gradient norms are about 6.5 and 6.3 (asserted).
MOE_MAX_GRAD_NORM = 0.1


def build_moe(mesh=None, axis=1, dtype=torch.float32, device=None):
    return MoEGPTModel(MOE_CFG, mesh, axis, dtype, device, init_seed=21)


def _train_moe(method, dp):
    """Clipped steps on the MoE model; returns (per-step last_grad_norm,
    the parameters outside the expert layers)."""
    state = aa.TrainState.create(build_moe, method, lr=1e-3,
                                 max_grad_norm=MOE_MAX_GRAD_NORM)
    step = aa.parallelize(lambda m, b: m.loss(b[0], b[1]), method=method)
    idx = state.mesh.axis_index(0) if dp > 1 else 0
    per = BATCH // dp
    norms = []
    for i in range(MOE_STEPS):
        g = torch.Generator().manual_seed(700 + i)
        ids = torch.randint(0, MOE_CFG.vocab_size, (BATCH, MOE_CFG.seq_len),
                            generator=g)
        labels = torch.randint(0, MOE_CFG.vocab_size,
                               (BATCH, MOE_CFG.seq_len), generator=g)
        step(state, (ids[idx * per:(idx + 1) * per],
                     labels[idx * per:(idx + 1) * per]))
        norms.append(state.optimizer.last_grad_norm.reshape(()).clone())
    params = [p.detach().clone() for n, p in
              state.model.named_parameters() if "moe" not in n]
    return torch.stack(norms), params


def test_clipped_ep2_matches_serial():
    """dp=ep=2: each rank owns half the experts and their gradients are not
    all-reduced, so the norm has to sum their squares over the ranks and
    count the replicated gradients once.  Every rank then clips by the
    serial run's norm and the replicas stay bit-identical."""
    serial_norms, serial_params = _train_moe(
        aa.ShardParallel(logical_mesh_shape=(1, 1)), 1)
    assert (serial_norms > MOE_MAX_GRAD_NORM).all(), serial_norms
    results = run_distributed(_worker, world_size=2, args=("ep",),
                              timeout=300)
    (norms0, params0), (norms1, params1) = results
    assert torch.equal(norms0, norms1), (norms0, norms1)
    for a, b in zip(params0, params1):
        assert torch.equal(a, b), "replicated parameters drifted apart"
    # tests/test_moe_cpu.py found the EP gradients equal to the serial ones
    # to 1e-5 relative (expert-GEMM summation order); a norm that leaves out
    # the other rank's experts is off by 2.5e-3
    torch.testing.assert_close(norms0, serial_norms, rtol=1e-4, atol=0)
    # parameters at that file's tolerance for this model
    for sp, rp in zip(serial_params, params0):
        torch.testing.assert_close(rp, sp, rtol=5e-2, atol=1e-3)
