"""dX of the linear layers through the weight's twin (TN GEMM on W.t()) and
through the weight (NN GEMM), both against an fp64 product of the same bf16
inputs, with dW and db bit-identical between the two routes.

Bound per element of dx = dy @ w, K = out_features terms: one bf16 rounding
of the result, 2^-8 |y64|, plus fp32 accumulation in any order,
K 2^-23 sum|a||b|.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd import ops
from alpa_amd.global_env import global_config

BF16 = torch.bfloat16


@pytest.fixture
def twin_switch():
    old = global_config.weight_twin
    yield
    global_config.weight_twin = old


def _case(M, N, K, bias, seed):
    """x [M, N] -> y [M, K] through w [K, N]; dx = dy @ w sums over K."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=gen).to(BF16).cuda().requires_grad_()
    w = torch.nn.Parameter((torch.randn(K, N, generator=gen) / K ** 0.5)
                           .to(BF16).cuda())
    b = torch.nn.Parameter(torch.randn(K, generator=gen).to(BF16).cuda()) \
        if bias else None
    dy = torch.randn(M, K, generator=gen).to(BF16).cuda()
    return x, w, b, dy


def _grads(x, w, b, dy):
    for t in (x, w, b):
        if t is not None:
            t.grad = None
    ops.linear_bias(x, w, b).backward(dy)
    torch.cuda.synchronize()
    return x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,K", [(64, 64), (200, 192)])
def test_dx_on_twin_and_on_weight(twin_switch, M, K, bias):
    N = 128
    x, w, b, dy = _case(M, N, K, bias, seed=M + K)
    assert ops.register_weight_twin(w) is not None
    y64 = dy.double() @ w.double()
    bound = 2.0 ** -8 * y64.abs() + \
        K * 2.0 ** -23 * (dy.double().abs() @ w.double().abs())
    got = {}
    for on in (True, False):
        global_config.weight_twin = on
        assert (ops.valid_weight_twin(w) is not None) == on
        dx, dw, db = _grads(x, w, b, dy)
        err = (dx.double() - y64).abs()
        print(f"twin={on} M={M} K={K}: max err/bound "
              f"{float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        got[on] = (dw, db)
    assert torch.equal(got[True][0].view(torch.int16),
                       got[False][0].view(torch.int16))
    if bias:
        assert torch.equal(got[True][1].view(torch.int16),
                           got[False][1].view(torch.int16))


def test_dx_reads_the_twin_only_when_the_switch_is_on(twin_switch):
    """A twin filled with something else and declared current: dx follows it
    with the switch on and ignores it with the switch off."""
    x, w, b, dy = _case(64, 128, 64, True, seed=11)
    twin = ops.register_weight_twin(w)
    global_config.weight_twin = False
    dx_w, _, _ = _grads(x, w, b, dy)
    dx_w = dx_w.clone()
    with torch.no_grad():
        twin.mul_(2.0)  # exact in bf16: dx doubles, exactly
    ops.weight_twin_written(w)
    dx_off, _, _ = _grads(x, w, b, dy)
    assert torch.equal(dx_off, dx_w)
    global_config.weight_twin = True
    dx_on, dw_on, _ = _grads(x, w, b, dy)
    assert not torch.equal(dx_on, dx_w)
    y64 = 2.0 * (dy.double() @ w.double())
    bound = 2.0 ** -8 * y64.abs() + \
        64 * 2.0 ** -23 * 2.0 * (dy.double().abs() @ w.double().abs())
    assert ((dx_on.double() - y64).abs() <= bound).all()


def test_stale_twin_is_rebuilt_in_eager_mode(twin_switch):
    global_config.weight_twin = True
    x, w, b, dy = _case(64, 128, 64, True, seed=7)
    twin = ops.register_weight_twin(w)
    with torch.no_grad():
        w.copy_(torch.randn_like(w))  # bumps w._version; the twin is stale
    assert not torch.equal(twin, w.t())
    dx, _, _ = _grads(x, w, b, dy)
    assert torch.equal(twin, w.t())
    y64 = dy.double() @ w.double()
    bound = 2.0 ** -8 * y64.abs() + \
        64 * 2.0 ** -23 * (dy.double().abs() @ w.double().abs())
    assert ((dx.double() - y64).abs() <= bound).all()
