"""Weight twins (ops.weight_twin): ownership, validity and the plumbing from
TrainState through AdamW to the linear layers' backward, on the CPU
reference path.  TrainState attaches twins by itself only on the GPU; here
the optimizer is asked to, which is the same call.
"""
import pytest
import torch

from dist_utils import run_distributed

import alpa_amd as aa
from alpa_amd import ops
from alpa_amd.global_env import global_config
from alpa_amd.models.gpt import Block, GPTConfig, GPTModel
from alpa_amd.serialization import restore_train_state, save_train_state

# bench.py's CPU configuration
CFG = GPTConfig(hidden_size=128, num_layers=2, num_heads=4, seq_len=64,
                vocab_size=512)
STEPS = 3


@pytest.fixture(autouse=True)
def twin_switch():
    old = global_config.weight_twin
    global_config.weight_twin = True
    yield
    global_config.weight_twin = old


def build(mesh=None, axis=1, dtype=torch.float32, device=None):
    torch.manual_seed(1234)
    return GPTModel(CFG, mesh, axis, dtype, device)


def _batch():
    g = torch.Generator().manual_seed(4321)
    ids = torch.randint(0, CFG.vocab_size, (4, CFG.seq_len), generator=g)
    labels = torch.randint(0, CFG.vocab_size, (4, CFG.seq_len), generator=g)
    return {"ids": ids, "labels": labels}


def _make(method=None, twins=True):
    method = method or aa.ShardParallel(logical_mesh_shape=(1, 1))
    state = aa.TrainState.create(build, method, lr=1e-3, weight_decay=0.01)
    if twins:
        assert state.optimizer.attach_weight_twins(state.model) > 0
    step = aa.parallelize(lambda m, b: m.loss(b["ids"], b["labels"]),
                          method=method)
    return state, step


def _twinned(model):
    return [(n, p, ops.weight_twin(p)) for n, p in model.named_parameters()
            if ops.weight_twin(p) is not None]


def _train(state, step, n=STEPS):
    batch = _batch()
    return torch.stack([step(state, batch).detach() for _ in range(n)])


def test_switch_on_and_off_agree():
    on_state, on_step = _make()
    losses_on = _train(on_state, on_step)
    global_config.weight_twin = False
    off_state, off_step = _make(twins=False)
    assert not _twinned(off_state.model)
    losses_off = _train(off_state, off_step)
    # the transposed CPU matmul may reorder sums: fp32 round-off only
    torch.testing.assert_close(losses_on, losses_off, rtol=1e-5, atol=1e-6)
    for (n, p), (_, q) in zip(on_state.model.named_parameters(),
                              off_state.model.named_parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5,
                                   atol=1e-6, msg=n)


def test_which_weights_get_a_twin_and_twins_follow_the_steps():
    state, step = _make()
    names = {n for n, _, _ in _twinned(state.model)}
    per_layer = {"attn.qkv.weight", "attn.out.weight", "mlp.fc1.weight",
                 "mlp.fc2.weight"}
    assert len(names) == 4 * CFG.num_layers + 1
    assert "lm_head.weight" in names and "wte.weight" not in names
    assert {n.split(".", 2)[2] for n in names
            if n.startswith("blocks.")} == per_layer
    _train(state, step)
    for n, p, t in _twinned(state.model):
        assert t.shape == (p.shape[1], p.shape[0]) and t.is_contiguous()
        assert torch.equal(t, p.t()), n


def test_twins_are_not_model_or_checkpoint_state(tmp_path):
    with_twins, step = _make()
    without, _ = _make(twins=False)
    assert [n for n, _ in with_twins.model.named_parameters()] == \
        [n for n, _ in without.model.named_parameters()]
    assert list(with_twins.model.state_dict()) == \
        list(without.model.state_dict())
    assert len(with_twins.optimizer.params) == len(without.optimizer.params)
    assert [b.numel for b in with_twins.grad_sync.buckets] == \
        [b.numel for b in without.grad_sync.buckets]
    save_train_state(str(tmp_path / "a"), with_twins, step=0)
    save_train_state(str(tmp_path / "b"), without, step=0)
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*")
                             if p.is_file())
    assert files(tmp_path / "a") == files(tmp_path / "b")
    # same seed, no step taken: the two checkpoints hold the same bytes
    for f in files(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == \
            (tmp_path / "b" / f).read_bytes(), f


def test_save_restore_then_step(tmp_path):
    state, step = _make()
    _train(state, step, 1)
    save_train_state(str(tmp_path), state, step=1)
    with torch.no_grad():
        for p in state.model.parameters():
            p.add_(1.0)
    restore_train_state(str(tmp_path), state, step=1)
    # the restore wrote the weights behind the optimizer's back: the twins
    # are stale now, and the next step must not use them as they are
    p0 = next(p for p in state.model.parameters()
              if id(p) in ops._WEIGHT_TWINS)
    assert not ops._WEIGHT_TWINS[id(p0)].is_current(p0)
    _train(state, step, 1)
    for n, p, t in _twinned(state.model):
        assert torch.equal(t, p.t()), n


def test_stale_twin_is_rebuilt_before_use():
    state, step = _make()
    n, p, t = _twinned(state.model)[0]
    entry = ops._WEIGHT_TWINS[id(p)]
    with torch.no_grad():
        p.copy_(torch.randn_like(p))
    assert not entry.is_current(p) and not torch.equal(entry.twin, p.t())
    assert torch.equal(ops.valid_weight_twin(p), p.t())
    assert entry.is_current(p)


def _zero_worker(rank, world_size, kind):
    """Counts what TrainState.create hands to the twin attachment, so the
    answer does not hang on this host having no GPU."""
    calls = []
    orig = aa.TrainState._attach_weight_twins
    aa.TrainState._attach_weight_twins = \
        lambda self: calls.append(type(self.optimizer).__name__)
    try:
        method = {"zero2": aa.Zero2Parallel, "zero3": aa.Zero3Parallel,
                  "dp": aa.DataParallel}[kind]()
        state, step = _make(method, twins=False)
    finally:
        aa.TrainState._attach_weight_twins = orig
    opt = state.optimizer
    holders = [o for o in (opt, getattr(opt, "rest_opt", None))
               if hasattr(o, "_twins")]
    loss = step(state, _batch())
    return (calls, any(o._twins for o in holders), len(ops._WEIGHT_TWINS),
            bool(torch.isfinite(loss)))


@pytest.mark.parametrize("kind", ["zero2", "zero3"])
def test_zero_states_attach_no_twins(kind):
    for calls, held, registered, finite in run_distributed(
            _zero_worker, world_size=2, args=(kind,)):
        assert calls == [] and not held and registered == 0 and finite


def test_dp_state_is_offered_twins():
    """The control for the test above: zero_stage 0 does reach the
    attachment."""
    for calls, _, _, finite in run_distributed(_zero_worker, world_size=2,
                                               args=("dp",)):
        assert calls == ["AdamW"] and finite


def test_fp8_and_memory_limit_attach_nothing(monkeypatch):
    state, _ = _make(twins=False)
    monkeypatch.setattr(global_config, "fp8_gemm", True)
    assert state.optimizer.attach_weight_twins(state.model) == 0
    monkeypatch.setattr(global_config, "fp8_gemm", False)
    monkeypatch.setattr(global_config, "weight_twin", False)
    assert state.optimizer.attach_weight_twins(state.model) == 0
    assert not ops._WEIGHT_TWINS or all(
        ops.weight_twin(p) is None for p in state.model.parameters())


def test_storage_swap_makes_the_twin_stale():
    state, _ = _make()
    _, p, _ = _twinned(state.model)[0]
    entry = ops._WEIGHT_TWINS[id(p)]
    p.data = torch.randn_like(p)  # same _version, other storage
    assert not entry.is_current(p)
    assert torch.equal(ops.weight_twin(p), p.t())
    p.data.mul_(2.0)  # in place through .data: not seen, as documented
    assert entry.is_current(p)
    ops.invalidate_weight_twin(p)
    assert torch.equal(ops.weight_twin(p), p.t())


def test_bare_optimizer_and_block_allocate_no_twin():
    block = Block(CFG, None, 1, torch.float32, None)
    opt = aa.AdamW(block.parameters())
    assert not opt._twins
    assert all(ops.weight_twin(p) is None for p in block.parameters())
