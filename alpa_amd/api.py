"""Top-level user API: init / shutdown / parallelize / TrainState.

Mirrors the reference's ``alpa/api.py`` surface (init:25, shutdown:63,
parallelize:71) with torch-idiomatic semantics: the user writes a
single-device loss function ``fn(model, batch) -> loss`` and decorates it;
the framework resolves a mesh from the ParallelMethod, builds/installs the
parallel execution machinery on first call (microbatch split, overlapped
grad collectives, fused optimizer), and runs the step SPMD on every rank.
"""
from __future__ import annotations

import functools
from typing import Any, Callable, Dict, List, Optional

import torch

from .global_env import global_config
from .mesh import (DeviceMesh, device, init_distributed, is_distributed,
                   rank, shutdown as _mesh_shutdown, world_size)
from .optim import AdamW, check_max_grad_norm
from .parallel.grad_sync import GradSynchronizer
from .parallel_method import ParallelMethod, ShardParallel


def init(cluster: str = "auto", backend: Optional[str] = None) -> None:
    """Bring up the distributed world (reference api.py:25 / device_mesh
    bring-up 3.1 — here just torch.distributed init, one process per GPU)."""
    init_distributed(backend=backend)


def shutdown() -> None:
    """Tear down the world (reference api.py:63)."""
    _mesh_shutdown()


class TrainState:
    """Model + fused optimizer + parallel wiring for one training job.

    Loose analog of the reference's TrainState + DistributedArray placement:
    in SPMD-per-rank execution the "placement" is simply which shard of each
    parameter this rank's model instance holds.
    """

    def __init__(self, model: torch.nn.Module, optimizer: AdamW,
                 method: ParallelMethod, mesh: Optional[DeviceMesh]):
        self.model = model
        self.optimizer = optimizer
        self.method = method
        self.mesh = mesh
        self.grad_sync: Optional[GradSynchronizer] = None
        self.engine = None  # PipelineEngine for PipeshardParallel
        self.step_count = 0
        #: optional fp16 loss scaling (dynamic_scale.DynamicScale);
        #: unused for the default bf16 compute dtype
        self.dynamic_scale = None

    @staticmethod
    def _check_clip_supported(max_grad_norm: Optional[float],
                              method: ParallelMethod,
                              mesh: Optional[DeviceMesh]) -> None:
        """Global-norm clipping needs the norm over every gradient of the
        model exactly once.  Serial, dp and ZeRO-2/3 runs can form it, and
        so can dp with expert parallelism (_expert_grad_groups); the
        layouts below cannot yet, and fail here instead of clipping by a
        wrong norm."""
        if max_grad_norm is None:
            return
        from .parallel_method import PipeshardParallel
        if isinstance(method, PipeshardParallel):
            raise NotImplementedError(
                "max_grad_norm is not supported with PipeshardParallel: each "
                "stage holds only its own gradients and there is no "
                "cross-stage reduction of their sum of squares yet")
        if mesh is not None and mesh.axis_size(method.tp_axis) > 1:
            raise NotImplementedError(
                "max_grad_norm is not supported with tp > 1: there is no "
                "registry yet of which parameters are TP-sharded (summed "
                "over tp ranks) and which are replicated (counted once), "
                "so the global gradient norm cannot be formed")

    @staticmethod
    def _expert_grad_groups(max_grad_norm: Optional[float],
                            model: torch.nn.Module,
                            method: ParallelMethod) -> dict:
        """{id(param): process group} for expert-parallel weights whose
        experts are spread over more than one rank.  Their gradients are
        not all-reduced (each rank owns other experts), so the clipping
        norm must sum their squares over that group, while every other
        gradient is replicated and counts once.  The ZeRO optimizers shard
        flat buckets without that distinction, so they refuse."""
        if max_grad_norm is None:
            return {}
        from .parallel.expert import ExpertParallelMLP
        groups = {}
        for mod in model.modules():
            if isinstance(mod, ExpertParallelMLP) and mod.ep > 1:
                group = mod.mesh.axis_group(mod.axis)
                for p in (mod.w1, mod.w2):
                    groups[id(p)] = group
        if groups and method.zero_stage >= 2:
            raise NotImplementedError(
                "max_grad_norm is not supported with expert parallelism "
                "under ZeRO-2/3: the sharded optimizers cannot tell "
                "rank-local expert gradients from replicated ones when "
                "they form the global gradient norm")
        return groups

    @classmethod
    def create(cls, model_fn, method: ParallelMethod, lr: float = 1e-4,
               betas=(0.9, 0.95), weight_decay: float = 0.0,
               optimizer_cls=AdamW,
               max_grad_norm: Optional[float] = None) -> "TrainState":
        """model_fn(mesh, axis, dtype, device) -> nn.Module built directly
        on the target device with method-resolved sharding; for
        PipeshardParallel, model_fn is a PipelineModelSpec instead.

        ``max_grad_norm`` clips the gradients by their global norm inside
        the fused AdamW step (optax ``clip_by_global_norm``); after a step
        ``state.optimizer.last_grad_norm`` holds the pre-clip norm on the
        device.  Supported for serial, dp (with or without expert
        parallelism), ZeRO-2 and ZeRO-3 runs."""
        from .parallel_method import PipeshardParallel
        check_max_grad_norm(max_grad_norm)
        cls._check_clip_supported(max_grad_norm, method, None)
        if isinstance(method, PipeshardParallel):
            from .pipeline_parallel.compile import build_pipeline_state
            stage_module, engine, opt, gs, meshes = build_pipeline_state(
                model_fn, method, lr, betas, weight_decay)
            state = cls(stage_module, opt, method, engine.mesh)
            state.engine = engine
            state.grad_sync = gs
            state.stage_meshes = meshes
            return state
        mesh = method.resolve_mesh()
        cls._check_clip_supported(max_grad_norm, method, mesh)
        dtype = getattr(torch, global_config.compute_dtype) \
            if torch.cuda.is_available() else torch.float32
        model = model_fn(mesh=mesh, axis=method.tp_axis, dtype=dtype,
                         device=device())
        expert_groups = cls._expert_grad_groups(max_grad_norm, model, method)
        state = cls(model, None, method, mesh)
        if method.zero_stage >= 3:
            state._install_zero3(lr, betas, weight_decay, max_grad_norm)
        elif method.zero_stage == 2:
            state._install_grad_sync()
            from .parallel.zero import ZeroOptimizer
            state.optimizer = ZeroOptimizer(state.grad_sync, lr=lr,
                                            betas=betas,
                                            weight_decay=weight_decay,
                                            max_grad_norm=max_grad_norm)
        else:
            state._install_grad_sync()
            # only pass the options where they are set: optimizer_cls may
            # be a user class without them
            clip = {}
            if max_grad_norm is not None:
                clip["max_grad_norm"] = max_grad_norm
            if expert_groups:
                clip["grad_norm_groups"] = expert_groups
            state.optimizer = optimizer_cls(model.parameters(), lr=lr,
                                            betas=betas,
                                            weight_decay=weight_decay,
                                            **clip)
        return state

    @classmethod
    def create_auto(cls, builder: Callable[[], torch.nn.Module],
                    example_inputs, method: Optional["ShardParallel"] = None,
                    lr: float = 1e-4, betas=(0.9, 0.95),
                    weight_decay: float = 0.0,
                    max_grad_norm: Optional[float] = None) -> "TrainState":
        """Automatic parallelization of an ARBITRARY plain torch module —
        no zoo membership, no model_hint (the reference's headline
        capability: trace any program and parallelize it,
        compile_shard_executable.py:54).

        ``builder()`` returns the plain model (seed inside the builder so
        every rank constructs identical weights); ``example_inputs`` is a
        tensor or tuple of tensors for one forward.  The model is traced
        (shard_parallel/capture.py), the ILP solves per-node strategies,
        and the plan is EXECUTED by converting the matched modules to
        parallel layers with automatic resharding on mismatched edges
        (shard_parallel/plan_apply.py).  The usual step machinery
        (microbatching, overlapped grad sync, fused AdamW) is installed
        on top, so `aa.parallelize(step_fn)` works unchanged.
        ``max_grad_norm`` is as in :meth:`create`; a plan that shards over
        tp raises NotImplementedError.
        """
        from .shard_parallel import auto_shard
        check_max_grad_norm(max_grad_norm)
        method = method or ShardParallel()
        model = builder()
        dtype = getattr(torch, global_config.compute_dtype) \
            if torch.cuda.is_available() else torch.float32
        model = model.to(device=device(), dtype=dtype)

        def to_dev(t):
            if torch.is_tensor(t):
                t = t.to(device())
                return t.to(dtype) if t.is_floating_point() else t
            return t
        if torch.is_tensor(example_inputs):
            example_inputs = (example_inputs,)
        example_inputs = tuple(to_dev(t) for t in example_inputs)
        o = method.auto_sharding_option
        model, plan, mesh = auto_shard(
            model, example_inputs,
            memory_budget=o.memory_budget_per_device,
            force_data_parallel=o.force_data_parallel,
            mesh_shape=method.logical_mesh_shape)
        method.logical_mesh_shape = plan.mesh_shape
        cls._check_clip_supported(max_grad_norm, method, mesh)
        expert_groups = cls._expert_grad_groups(max_grad_norm, model, method)
        state = cls(model, None, method, mesh)
        state.plan = plan
        state._install_grad_sync()
        state.optimizer = AdamW(model.parameters(), lr=lr, betas=betas,
                                weight_decay=weight_decay,
                                max_grad_norm=max_grad_norm,
                                grad_norm_groups=expert_groups or None)
        return state

    def _install_zero3(self, lr, betas, weight_decay, max_grad_norm=None):
        """ZeRO-3: block params sharded + JIT-gathered (parallel/zero3.py);
        leftover params (e.g. positional embeddings) use plain DP sync."""
        from .parallel.zero3 import Zero3Manager, Zero3Optimizer
        model, m = self.model, self.method
        if hasattr(model, "zero3_blocks"):
            blocks = model.zero3_blocks()
        else:
            blocks = []
            for child in model.children():
                if isinstance(child, torch.nn.ModuleList):
                    blocks.extend(child)
                elif any(p.requires_grad for p in child.parameters()):
                    blocks.append(child)
        # drop blocks whose params are already covered (tied weights)
        seen = set()
        uniq = []
        for b in blocks:
            ps = [p for p in b.parameters() if p.requires_grad and
                  id(p) not in seen]
            if ps:
                uniq.append(b)
                seen.update(id(p) for p in ps)
        manager = Zero3Manager(uniq, self.mesh, axis=m.dp_axis)
        rest = [p for p in model.parameters()
                if p.requires_grad and id(p) not in manager._by_param]
        self.grad_sync = GradSynchronizer(rest, self.mesh, axis=m.dp_axis)
        z3 = Zero3Optimizer(manager, lr=lr, betas=betas,
                            weight_decay=weight_decay,
                            max_grad_norm=max_grad_norm)
        rest_opt = AdamW(rest, lr=lr, betas=betas,
                         weight_decay=weight_decay,
                         max_grad_norm=max_grad_norm) if rest else None
        state_self = self

        class _Composite:

            def __init__(self):
                self.step_count = 0
                # exposed for checkpointing (serialization.py saves the
                # sharded moments of both halves)
                self.z3 = z3
                self.rest_opt = rest_opt
                self.max_grad_norm = max_grad_norm
                self.last_grad_norm = None

            def step(self, grads=None, grad_scale: float = 1.0,
                     grad_sumsq=None):
                if max_grad_norm is not None and grad_sumsq is None:
                    # one global coefficient for both halves: the shards'
                    # sum over dp plus the replicated rest's, counted once
                    from . import ops
                    grad_sumsq = z3.shard_sumsq()
                    rest_grads = [p.grad for p in rest_opt.params
                                  if p.grad is not None] if rest_opt else []
                    if rest_grads:
                        grad_sumsq = grad_sumsq + \
                            ops.multi_tensor_sumsq(rest_grads)
                z3.step(grad_scale=grad_scale, grad_sumsq=grad_sumsq)
                if rest_opt is not None:
                    rest_opt.step(grad_scale=grad_scale,
                                  grad_sumsq=grad_sumsq)
                self.last_grad_norm = z3.last_grad_norm
                # shard grads accumulated across microbatches: clear for
                # the next step
                manager.zero_grads()
                self.step_count += 1

            def zero_grad(self):
                manager.zero_grads()

            def state_dict(self):
                sd = {"zero3": z3.state_dict(), "step": self.step_count}
                if rest_opt is not None:
                    sd["rest"] = rest_opt.state_dict()
                return sd

            def load_state_dict(self, sd):
                z3.load_state_dict(sd["zero3"])
                if rest_opt is not None and "rest" in sd:
                    rest_opt.load_state_dict(sd["rest"])
                self.step_count = sd.get("step", 0)

        self.zero3_manager = manager
        self.optimizer = _Composite()

    def _install_grad_sync(self):
        m = self.method
        params = list(self.model.parameters())
        self.grad_sync = GradSynchronizer(
            params, self.mesh, axis=m.dp_axis,
            reduce_scatter=(m.zero_stage >= 2))


def _split_microbatches(batch: Any, n: int) -> List[Any]:
    """Split every tensor leaf of `batch` into n chunks along dim 0."""
    if n == 1:
        return [batch]
    if torch.is_tensor(batch):
        assert batch.shape[0] % n == 0, \
            f"batch dim {batch.shape[0]} not divisible by {n} microbatches"
        return list(batch.chunk(n, dim=0))
    if isinstance(batch, dict):
        split = {k: _split_microbatches(v, n) for k, v in batch.items()}
        return [{k: v[i] for k, v in split.items()} for i in range(n)]
    if isinstance(batch, (list, tuple)):
        split = [_split_microbatches(v, n) for v in batch]
        return [type(batch)(s[i] for s in split) for i in range(n)]
    raise TypeError(f"unsupported batch leaf {type(batch)}")


class ParallelizedFunc:
    """The compiled step callable (reference ParallelizedFunc, api.py:106).

    Hot path per call (shard-parallel):
      for each microbatch: forward -> backward (grad collectives overlapped,
      gated to the last microbatch); then one fused AdamW launch with the
      1/(nmb*dp) scale folded in.
    """

    def __init__(self, fn: Callable, method: ParallelMethod):
        self.fn = fn
        self.method = method
        self._compiled = False

    def __call__(self, state: TrainState, batch: Any) -> torch.Tensor:
        m = self.method
        nmb = m.num_micro_batches
        micro = _split_microbatches(batch, nmb)
        if state.engine is not None:
            return self._pipeline_call(state, micro)
        gs = state.grad_sync
        ds = state.dynamic_scale
        gs.zero_grads()
        total_loss = None
        for i, mb in enumerate(micro):
            gs.begin_microbatch(is_last=(i == nmb - 1))
            loss = self.fn(state.model, mb)
            (ds.scale_loss(loss) if ds is not None else loss).backward()
            total_loss = loss.detach() if total_loss is None \
                else total_loss + loss.detach()
        gs.finish()
        # grad scale: mean over microbatches; all-reduce over dp was a SUM
        dp = state.mesh.axis_size(m.dp_axis) if state.mesh is not None else 1
        scale = 1.0 / (nmb * (dp if dp > 1 else 1))
        if ds is not None:
            # fold the loss-scale unscale into the fused AdamW launch;
            # overflow => skip the update + back off (reference
            # DynamicScale, model_util.py).  The flag is made globally
            # consistent with an all-reduce MAX over the FULL mesh group:
            # under TP the per-rank weight-shard grads differ, and the
            # reference computes the is-finite reduction inside the SPMD
            # program for the same reason.  A local non-finite grad
            # implies a non-finite reduced grad (inf/nan propagate
            # through the sum), so scanning local views stays sound
            # under ZeRO-2 bucket sharding too.
            local_inf = ds.found_inf(
                p.grad for p in state.model.parameters())
            if is_distributed() and state.mesh is not None:
                import torch.distributed as dist
                flag = torch.tensor(
                    [1.0 if local_inf else 0.0],
                    device=device() if torch.cuda.is_available() else "cpu")
                state.mesh.all_reduce(flag, axis=None, op=dist.ReduceOp.MAX)
                local_inf = bool(flag.item() > 0)
            if ds.update(local_inf):
                gs.zero_grads()
                state.step_count += 1
                return total_loss / nmb
            scale *= ds.unscale_factor()
        state.optimizer.step(grad_scale=scale)
        state.step_count += 1
        return total_loss / nmb

    def _pipeline_call(self, state: TrainState, micro) -> torch.Tensor:
        """Pipeshard path: 1F1B engine step + per-stage fused optimizer +
        loss broadcast from the last stage."""
        import torch.distributed as dist
        m = self.method
        engine = state.engine
        loss = engine.train_step(micro)
        dp = getattr(engine, "loss_dp", engine.mesh.axis_size(m.dp_axis))
        scale = 1.0 / (m.num_micro_batches * (dp if dp > 1 else 1))
        state.optimizer.step(grad_scale=scale)
        state.step_count += 1
        if is_distributed():
            loss = loss.contiguous()
            dist.broadcast(loss, src=engine.loss_src_rank)
        return loss


def parallelize(fn: Optional[Callable] = None, *,
                method: Optional[ParallelMethod] = None):
    """Decorator: fn(model, microbatch) -> scalar loss  =>  step(state, batch).

    (reference api.py:71 `@parallelize`)
    """
    method = method or ShardParallel()

    def wrap(f):
        pf = ParallelizedFunc(f, method)
        functools.update_wrapper(pf, f, updated=[])
        return pf

    if fn is None:
        return wrap
    return wrap(fn)


def value_and_grad(fn: Callable):
    """Functional helper mirroring the reference's ``alpa.value_and_grad``
    (api.py:241): ``vg(model, batch) -> (loss, {name: grad})`` without
    touching ``.grad`` accumulation state (grads come from autograd.grad).
    The decorated training step (`parallelize`) does NOT need this; it
    exists for eval/diagnostic code written in the reference's style."""

    def vg(model: torch.nn.Module, batch):
        params = [p for p in model.parameters() if p.requires_grad]
        loss = fn(model, batch)
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        named = {}
        it = iter(grads)
        for n, p in model.named_parameters():
            if p.requires_grad:
                named[n] = next(it)
        return loss.detach(), named

    return vg


def grad(fn: Callable):
    """``alpa.grad`` analog (api.py:241): returns only the grads dict."""
    _vg = value_and_grad(fn)

    def g(model, batch):
        return _vg(model, batch)[1]

    return g
