"""Global configuration singleton.

MI355X-native analog of the reference's ``alpa/global_env.py:5`` GlobalConfig:
a single mutable options object read throughout the framework, with env-var
overrides.  Unlike the reference there is no Ray worker push — every rank
constructs the same config from its own environment (one process per GPU).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field


def _env_bool(name: str, default: bool) -> bool:
    v = os.environ.get(name)
    if v is None:
        return default
    return v.lower() not in ("0", "false", "no", "off")


@dataclass
class GlobalConfig:
    # ---------- backend ----------
    #: "hip" on a GPU box, "cpu" for GPU-free tests (gloo collectives).
    backend: str = "hip"
    #: torch.distributed backend name. "nccl" IS RCCL on ROCm.
    dist_backend: str = "auto"  # auto -> nccl if cuda available else gloo

    # ---------- compute ----------
    #: default compute dtype for models/benchmarks
    compute_dtype: str = "bfloat16"
    #: fp8(e4m3) GEMMs in the parallel linear layers with delayed
    #: scaling (fwd + backward; ops/fp8.py).  NOT valid for BASELINE
    #: comparisons (bf16 contract) — env ALPA_AMD_FP8=1
    fp8_gemm: bool = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_FP8", "0") == "1")
    #: compute dW in fp8 too (default); ALPA_AMD_FP8_WGRAD=0 keeps the
    #: weight-grad GEMM in bf16 (tighter numerics, ~1/3 less fp8 win)
    fp8_wgrad: bool = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_FP8_WGRAD",
                                               "1") == "1")
    #: hand-written decode GEMV (ops/csrc/skinny_gemm.hip) for
    #: inference GEMMs with <= 8 tokens.  "auto" (default) enables it
    #: only inside the MEASURED end-to-end win envelope — hidden-5120-
    #: class shapes (K <= 5120 or the matching 4x ffn K), where OPT-13B
    #: decode drops 11.85 -> 8.58 ms/token bf16 / 7.70 fp8.  hipBLASLt
    #: already streams >= 5 TB/s at hidden >= 7168 (30B/66B measured
    #: parity-to-loss end-to-end), so those stay on the library.
    #: ALPA_AMD_SKINNY=1 forces it everywhere, =0 disables.
    skinny_gemm: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_SKINNY",
                                               "auto"))
    #: split-KV decode attention (ops/csrc/attention_decode.hip) for
    #: single-token queries: ops.flash_attention at S_q == 1 outside
    #: autograd and ops.flash_attention_varlen.  "auto" (default) means
    #: on, everywhere inside the kernel's envelope (ops.decode_attn_ok):
    #: tools/decode_attn_bench.py measured it against the path it replaces
    #: (prefill kernel with kv_lens; blocked hipBLASLt path at head_dim
    #: 256) on the OPT-13B/30B, BLOOM-7.1B and CodeGen-16B head shapes at
    #: batch 1/8/32, lengths 128/512/2048, with and without 2048 keys of
    #: capacity, and it was faster in all 60 rows, in all by more than the
    #: round-to-round spread but one: 1.5-10x at batch 1, 2.2-3.4x on the
    #: HBM-bound OPT/BLOOM rows, 1.2-1.5x on the HBM-bound CodeGen rows,
    #: 3.7-9.3x at head_dim 128 with capacity beyond the slot length.  The exception
    #: (CodeGen, batch 32, length 128 of 2048: 1.11x, spread 0.27) has no
    #: other route: kv_lens at head_dim 256 exists in this kernel only.
    #: Table in docs/BENCHMARK.md, "Decode attention".  End to end
    #: (serve_bench, prompt 128): OPT-13B batch 32 12.50 -> 10.98 ms/token,
    #: CodeGen-16B batch 8 14.02 -> 11.39, OPT-13B batch 1 unchanged;
    #: OPT-13B batch 1 at prompt 1920: 12.30 -> 8.9.
    #: ALPA_AMD_DECODE_ATTN=1 is the same as auto, =0 restores the prefill
    #: kernel / blocked path.
    decode_attention: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_DECODE_ATTN",
                                               "auto"))

    #: compute dX with the bf16 MASTER weight instead of the fp8 wqt
    #: cache: halves the fp8 weight-cache footprint (the +30 GB dual
    #: cache at 15B pushes hipGraph capture OOM -> eager, see
    #: profiles/gpt15b_fp8_eager_diag_r02).  bench.py flips this on for
    #: >= 8B-param models; ALPA_AMD_FP8_DX_BF16=1 forces it
    fp8_dx_bf16: bool = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_FP8_DX_BF16",
                                               "0") == "1")
    #: emit the fp8 GEMM operands straight from the LayerNorm and
    #: bias+GeLU forward kernels (ops/csrc/fp8_fused.hip) instead of
    #: writing the bf16 activation and quantizing it in a second pass.
    #: Taken only under fp8_gemm with fp8_wgrad on and grad mode on;
    #: bit-identical to the two-pass path and measured faster (GPT-2.6B
    #: fp8 step 435 -> 426 ms, docs/BENCHMARK.md), so on by default.
    #: ALPA_AMD_FP8_FUSED_QUANT=0 keeps the two-pass path
    fp8_fused_quant: bool = field(
        default_factory=lambda: _env_bool("ALPA_AMD_FP8_FUSED_QUANT", True))
    #: route MoE tokens through the fused HIP kernels (top-2 gate, capacity
    #: slots, dispatch, combine; ops/csrc/moe_route.hip) when the input is
    #: inside their envelope (ops.moe_fused_ok).  They never read the
    #: device back, unlike the torch-op path with its data-dependent
    #: shapes.  ALPA_AMD_MOE_FUSED=0 keeps the torch-op path everywhere
    moe_fused_routing: bool = field(
        default_factory=lambda: _env_bool("ALPA_AMD_MOE_FUSED", True))
    #: scatter-allgather resharding rewrite at replicated stage
    #: boundaries (ship 1/R per replica + intra-group all-gather;
    #: reference use_local_allgather, global_env.py:72)
    use_local_allgather: bool = True
    #: use hand-written HIP kernels when their extension is available
    use_hip_kernels: bool = True
    #: fail loudly if running on GPU without the HIP extension (anti-silent-fallback)
    require_hip_kernels_on_gpu: bool = True
    #: capture the steady-state step in a hipGraph when possible
    #: (single mesh, no collectives inside the graph; bench.py consults
    #: this in addition to its --no-hipgraph flag)
    use_hip_graphs: bool = True

    # ---------- collectives ----------
    #: bucket size for gradient all-reduce / reduce-scatter (bytes).
    #: xGMI rings are per-link bound (~153 GB/s); larger buckets amortize
    #: launch + ring latency. 100 MiB default.
    grad_bucket_bytes: int = 100 * 1024 * 1024
    #: overlap grad collectives with backward
    overlap_grad_sync: bool = True
    #: alpha (s) and beta (s/byte) for the mesh cost model, calibrated for
    #: single-node xGMI (ring all-reduce is bound by one ~153 GB/s link).
    mesh_alpha: float = 1e-5
    mesh_beta: float = 1.0 / (150e9)

    # ---------- auto-sharding ----------
    #: ILP time limit (s) for scipy/HiGHS
    solver_timeout: float = 600.0
    #: memory budget fraction of HBM used by the ILP memory constraint
    memory_fraction: float = 0.9
    #: print chosen strategies (debug)
    print_strategy: bool = _env_bool("ALPA_AMD_DEBUG_PRINT_STRATEGY", False)

    # ---------- pipeline ----------
    pipeline_check_alive: bool = True
    collect_trace: bool = False

    # ---------- benchmark ----------

    # ---------- paths ----------
    prof_database_path: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_PROF_DB", "prof_database.pkl"))

    def resolved_dist_backend(self) -> str:
        if self.dist_backend != "auto":
            return self.dist_backend
        import torch
        return "nccl" if torch.cuda.is_available() else "gloo"


global_config = GlobalConfig()
