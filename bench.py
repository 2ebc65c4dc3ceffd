"""Flagship training benchmark — GPT-2.6B (BASELINE.md headline config).

Driver contract:
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
(N>1 launched via torch.distributed.run, one rank per GPU over RCCL.)

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print one JSON result line.  ``--dump-outputs DIR`` additionally
writes what the last timed step produced (see _dump_outputs) so two builds
can be compared output for output; inputs and initial weights are seeded and
identical from run to run.  ``--full`` is where any extra measurement beyond
the headline (baselines, other precisions/sizes, per-kernel figures) belongs;
today the benchmark has none, so it changes nothing.

Measures Alpa's headline metric on Alpa's headline config: model TFLOPS for
GPT-2.6B (H=2560, L=32, heads=32, vocab 51200, seq 1024), batch 32 per GPU,
bf16, synthetic data, random-init weights.  Microbatching defaults to 1
(no pipeline here; the reference's nmb=4 belongs to its dp2xop2xpp2
plan — see --nmb).  TFLOPS
accounting follows the reference formula exactly
(``benchmark/alpa/util.py:65-89``):
  factor*B*S*H^2*L*(1+S/(6H)) + 6*B*S*H*V, factor=72 fwd+bwd (96 w/ remat).
Baseline: 37.01 TFLOPS/GPU x 8 = 296 TFLOPS aggregate on 8x V100
(benchmark/alpa/README.md:89-101).
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

import alpa_amd as aa
from alpa_amd.models.gpt import GPTConfig, GPTModel, gpt_config


def model_tflops_per_step(cfg: GPTConfig, global_batch: int,
                          remat: bool = False) -> float:
    B, S, H, L, V = (global_batch, cfg.seq_len, cfg.hidden_size,
                     cfg.num_layers, cfg.vocab_size)
    factor = 96 if remat else 72
    return (factor * B * S * H * H * L * (1 + S / (6 * H)) +
            6 * B * S * H * V) / 1e12


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--model", type=str, default="auto",
                   help="GPT spec name (125M..76B) or 'auto'")
    p.add_argument("--batch-per-gpu", type=int, default=32)
    p.add_argument("--nmb", type=int, default=0,
                   help="num micro batches; 0 = auto (1: without a "
                        "pipeline, microbatching only shrinks GEMMs — "
                        "measured 760 vs 738 TF — and grad-sync overlap "
                        "spans the whole backward)")
    p.add_argument("--dp", type=int, default=0, help="data-parallel degree "
                   "(0 = all GPUs)")
    p.add_argument("--tp", type=int, default=1, help="tensor-parallel degree")
    p.add_argument("--parallel", choices=["auto", "manual"], default="auto",
                   help="auto = ILP auto-sharding picks (dp, tp)")
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--remat", action="store_true",
                   help="activation remat at block boundaries (TFLOPS "
                        "accounting then uses the reference's factor 96)")
    p.add_argument("--no-hipgraph", action="store_true",
                   help="disable hipGraph step capture (single-GPU only)")
    p.add_argument("--fp8", action="store_true",
                   help="fp8 (e4m3) GEMMs with delayed scaling for all "
                        "linear fwd+bwd (ops/fp8.py).  NOT the headline "
                        "metric: BASELINE requires bf16 compute; this "
                        "reports dtype=bf16+fp8gemm for comparison")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write the outputs of the "
                        "last timed step (loss + a seeded sample of the "
                        "updated parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run every measurement beyond the headline "
                        "figure (none today: the plain run is already just "
                        "setup + warmup + timed steps)")
    args = p.parse_args()
    assert args.steps >= 1, "--steps must be >= 1"
    if args.nmb == 0:
        args.nmb = 1
    return args


def _enable_tunableop():
    """Load the shipped hipBLASLt TunableOp selections for gfx950 (tuned
    once on MI355X; ~2% over the default heuristics)."""
    base = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "alpa_amd", "ops", "tuned", "tunableop_gfx950_.csv")
    if os.path.exists(base.replace("_.csv", "_0.csv")):
        os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
        os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", base)


#: per-parameter sample size for --dump-outputs (GPT-2.6B: ~390 tensors
#: x 16384 x 4 B = ~26 MB, well under the 64 MB cap)
_DUMP_SAMPLE = 16384
_DUMP_MAX_BYTES = 64 * 2**20


def _dump_outputs(out_dir: str, loss: torch.Tensor, model) -> None:
    """Write what a caller of the timed step receives from its last call:
    the returned loss, and the parameters the step updated in place.  The
    parameters are too large to dump whole, so each tensor contributes a
    fixed, seeded sample of its elements (all of them when it is small),
    concatenated in named_parameters() order.  Everything is float32."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().cpu().numpy().reshape(1))
    g = torch.Generator().manual_seed(97531)
    params = list(model.named_parameters())
    per = min(_DUMP_SAMPLE,
              max(1, (_DUMP_MAX_BYTES - 4) // (4 * max(len(params), 1))))
    chunks = []
    for _, p in params:
        flat = p.detach().reshape(-1)
        if flat.numel() > per:
            idx = torch.randint(0, flat.numel(), (per,), generator=g)
            flat = flat[idx.to(flat.device)]
        chunks.append(flat.float().cpu())
    sample = torch.cat(chunks) if chunks else torch.zeros(0)
    np.save(os.path.join(out_dir, "params_sample.npy"), sample.numpy())


def main():
    args = parse_args()
    if torch.cuda.is_available():
        _enable_tunableop()
    if args.fp8:
        from alpa_amd.global_env import global_config as _gc0
        _gc0.fp8_gemm = True
        # huge models: dX on the bf16 master weight so the fp8 weight
        # cache halves and hipGraph capture fits (see global_env)
        try:
            # gpt_config is the module-level import — re-importing it
            # here would shadow it for the whole function
            if torch.cuda.is_available() and args.model != "auto" and \
                    gpt_config(args.model).num_params() > 8e9:
                _gc0.fp8_dx_bf16 = True
        except Exception:
            pass
    aa.init()
    on_gpu = torch.cuda.is_available()
    n = aa.world_size()
    assert n == args.gpus or args.gpus == 1 or not on_gpu, \
        f"world_size {n} != --gpus {args.gpus}"
    n = max(n, 1)

    model_name = args.model
    if model_name == "auto":
        model_name = "2.6B" if on_gpu else "125M"
    if on_gpu:
        cfg = gpt_config(model_name, seq_len=args.seq)
        cfg.remat = args.remat
        batch_per_gpu = args.batch_per_gpu
    else:
        # CPU smoke: tiny shapes so the script works without a GPU
        cfg = GPTConfig(hidden_size=128, num_layers=2, num_heads=4,
                        seq_len=64, vocab_size=512)
        batch_per_gpu = 4

    if args.parallel == "auto" and args.dp == 0 and n > 1:
        # ILP auto-sharding picks (dp, tp) from the op graph + xGMI costs.
        # Solve on rank 0 only and broadcast: every rank must construct the
        # same mesh (group creation is collective).
        state_bytes = 12.0 * cfg.num_params()
        hint = {
            "family": "gpt", "hidden": cfg.hidden_size,
            "layers": cfg.num_layers, "vocab": cfg.vocab_size,
            "tokens": args.batch_per_gpu * n * cfg.seq_len // args.nmb,
            "memory_budget": (0.9 * 288e9
                              if state_bytes > 0.5 * 288e9 else None),
        }
        from alpa_amd.shard_parallel.mesh_search import choose_mesh_shape
        probe = aa.ShardParallel(num_micro_batches=args.nmb,
                                 model_hint=hint)
        shape = choose_mesh_shape(probe, n) if aa.rank() == 0 else None
        if aa.world_size() > 1:
            import torch.distributed as dist
            lst = [shape]
            dist.broadcast_object_list(lst, src=0)
            shape = tuple(lst[0])
        dp, tp = shape
        method = aa.ShardParallel(num_micro_batches=args.nmb,
                                  logical_mesh_shape=(dp, tp))
    else:
        dp = args.dp if args.dp > 0 else n // args.tp
        tp = args.tp
        assert dp * tp == n, (dp, tp, n)
        method = aa.ShardParallel(num_micro_batches=args.nmb,
                                  logical_mesh_shape=(dp, tp))

    def build(mesh=None, axis=1, dtype=torch.float32, device=None):
        torch.manual_seed(1234)
        return GPTModel(cfg, mesh, axis, dtype, device)

    state = aa.TrainState.create(build, method, lr=1e-4, weight_decay=0.01)
    step_fn = aa.parallelize(
        lambda model, b: model.loss(b["ids"], b["labels"]), method=method)

    # synthetic data of the benchmark shape, one local batch per dp rank
    # (tp ranks of the same dp group must see identical data)
    mesh = state.mesh
    dp_idx = mesh.axis_index(0) if mesh is not None and mesh.is_member else 0
    g = torch.Generator().manual_seed(4321 + max(dp_idx, 0))
    ids = torch.randint(0, cfg.vocab_size, (batch_per_gpu, cfg.seq_len),
                        generator=g)
    labels = torch.randint(0, cfg.vocab_size, (batch_per_gpu, cfg.seq_len),
                           generator=g)
    dev = aa.device()
    batch = {"ids": ids.to(dev), "labels": labels.to(dev)}

    def sync():
        if mesh is not None:
            mesh.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        loss = step_fn(state, batch)

    # hipGraph capture of the whole training step (single GPU: no RCCL ops
    # in the graph).  The BASELINE north star's "HIP streams and graphs"
    # execution mode: after capture, one replay = fwd+bwd x nmb + fused
    # AdamW with zero host-side dispatch.
    graph = None
    from alpa_amd.global_env import global_config as _gc
    if (on_gpu and aa.world_size() == 1 and not args.no_hipgraph
            and _gc.use_hip_graphs):
        try:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                loss = step_fn(state, batch)
            graph.replay()  # one warm replay
            torch.cuda.synchronize()
        except Exception as e:
            print(f"# hipGraph capture unavailable ({e}); eager steps")
            graph = None

    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if graph is not None:
            graph.replay()
        else:
            loss = step_fn(state, batch)
    sync()
    elapsed = time.perf_counter() - t0
    # MAX over ranks
    et = torch.tensor([elapsed], dtype=torch.float64)
    if aa.world_size() > 1:
        import torch.distributed as dist
        et_d = et.to(dev) if on_gpu else et
        dist.all_reduce(et_d, op=dist.ReduceOp.MAX)
        elapsed = float(et_d.item())

    if args.dump_outputs and aa.rank() == 0:
        _dump_outputs(args.dump_outputs, loss, state.model)

    ms_per_step = elapsed / args.steps * 1000
    global_batch = batch_per_gpu * dp
    tflops_step = model_tflops_per_step(cfg, global_batch, args.remat)
    value = tflops_step / (elapsed / args.steps)  # aggregate TFLOPS
    baseline_aggregate_tflops = 296.0  # 37.01 TF/GPU x 8 V100

    if aa.rank() == 0:
        result = {
            "metric": "model_tflops_aggregate",
            "value": round(value, 2),
            "unit": "TFLOPS",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / baseline_aggregate_tflops, 3)
                           if on_gpu else None,
            "dtype": ("bf16+fp8gemm" if args.fp8 else "bf16")
                     if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"GPT-{model_name}" if on_gpu else "GPT-tiny-cpu",
                "hidden": cfg.hidden_size, "layers": cfg.num_layers,
                "heads": cfg.num_heads, "vocab": cfg.vocab_size,
                "global_batch": global_batch, "seq_len": cfg.seq_len,
                "num_micro_batches": args.nmb,
                "parallelism": f"dp{dp}" + (f"tp{tp}" if tp > 1 else ""),
                "auto_sharded": args.parallel == "auto",
                "hip_graph": graph is not None,
                "loss": float(loss),
            },
        }
        print(json.dumps(result))
    aa.shutdown()


if __name__ == "__main__":
    main()
