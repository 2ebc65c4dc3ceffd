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
    #: inference GEMMs with <= 8 tokens (9..64: below).  "auto" (default) enables it
    #: only inside the MEASURED end-to-end win envelope — hidden-5120-
    #: class shapes (K <= 5120 or the matching 4x ffn K), where OPT-13B
    #: decode drops 11.85 -> 8.58 ms/token bf16 / 7.70 fp8.  hipBLASLt
    #: already streams >= 5 TB/s at hidden >= 7168 (30B/66B measured
    #: parity-to-loss end-to-end), so those stay on the library.
    #: For 9..64 tokens the MFMA skinny GEMM (ops/csrc/skinny_mfma.hip)
    #: serves the same packed weights inside its envelope (N % 64 == 0,
    #: K % 256 == 0).  "auto" adds it on top of the rules above only
    #: where tools/skinny_bench.py measured a win over the library's bf16
    #: GEMM beyond the 6 % run-to-run spread (best legal split, two
    #: passes, M = 16/32/64; docs/BENCHMARK.md, "MFMA skinny GEMM"):
    #:   - K >= 2N (5120x20480): all tiers, 1.66-1.90x bf16, 2.12-2.95x
    #:     e4m3;
    #:   - e4m3 weights (fp8_gemm), any other shape: up to 32 tokens
    #:     (1.15-2.69x); 33..64 stay on the library (0.81-1.09x);
    #:   - bf16, N <= K (5120x5120): up to 32 tokens (1.16-1.34x);
    #:     33..64 stay on the library (0.94-0.98x);
    #:   - bf16, N > K (qkv 15360x5120, fc1 20480x5120) stays on the
    #:     library: 0.66-0.98x, except 1.78x at exactly M = 16 on fc1.
    #: End to end (serve_bench) was not measured for these batch sizes.
    #: ALPA_AMD_SKINNY=1 forces both kernels everywhere inside their
    #: envelopes, =0 disables both.
    skinny_gemm: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_SKINNY",
                                               "auto"))
    #: MXFP4 weight-only decode GEMMs: ops.skinny_linear packs every
    #: module that is not _fp8_exclude (so not the LM head) as e2m1
    #: nibbles with one e8m0 scale per 32 k (4.25 bits a weight) and runs
    #: ops/csrc/skinny_fp4.hip (up to 8 tokens) or skinny_mfma_fp4.hip
    #: (9..64); activations stay bf16 and the nibbles are dequantized
    #: exactly in registers, so the only error is the quantizer's.  It
    #: goes before fp8_gemm on the skinny path only: prefill and training
    #: are untouched.  K % 256 == 0 at every token count.  In skinny_gemm
    #: "auto" it follows the e4m3 rules above (the hidden >= 7168
    #: exception, the 9..64-token tiers).  Measured (tools/skinny_bench.py,
    #: docs/BENCHMARK.md, "MXFP4 weight-only kernels", four hidden-5120
    #: shapes): 9..32 tokens 1.09-1.35x over e4m3 and 1.36-3.68x over the
    #: library; 33..64 tokens level with e4m3, the library ahead at N > K
    #: as for e4m3, so that tier's rule stands; 4 tokens 1.07-1.29x over
    #: e4m3; 8 tokens level, and 0.91x of e4m3 at 20480x5120 (issue-bound).
    #: The hidden >= 7168 exception is by analogy with e4m3, NOT MEASURED
    #: for fp4, and neither is anything end to end.  Off by default;
    #: ALPA_AMD_FP4=1 turns it on.
    weight_fp4: bool = field(
        default_factory=lambda: _env_bool("ALPA_AMD_FP4", False))
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

    #: e4m3 KV cache for the cached decoders (models/decoder.py): KVCache
    #: holds bytes plus one fp32 scale per cached row (per slot, head and
    #: position; no calibration), rows are written by the fused
    #: quantize-and-append kernel (ops/csrc/kv_cache_fp8.hip) and read by
    #: the e4m3 split-KV decode kernel (ops/csrc/attention_decode_fp8.hip).
    #: Prefill attends over the fresh bf16 k/v as before.  Half the cache
    #: memory and half the bytes a decode step streams, at the cost of
    #: e4m3 rounding of k and v (docs/KERNELS.md, "e4m3 KV cache").
    #: tools/decode_attn_bench.py on one MI355X (table in
    #: docs/BENCHMARK.md, "e4m3 KV cache"): against the bf16 decode kernel
    #: the e4m3 one is 1.83-1.91x at batch 32, length 2048 (OPT-13B heads:
    #: 243.9 -> 130.7 us; spread 0.01-0.16) and 1.45-1.92x at batch 8,
    #: length 2048; parity to 1.3x at batch 1; 0.93-0.98x where 2048 keys
    #: of capacity hold 128-key slots at head_dim 128 (dispatch-bound).  The
    #: fused append takes 3.3-4.0 us against 11.5-14.9 us for the two
    #: index_put scatters.  End to end (serve_bench) was not measured.
    #: Off by default; ALPA_AMD_KV_FP8=1 turns it on.
    kv_cache_fp8: bool = field(
        default_factory=lambda: _env_bool("ALPA_AMD_KV_FP8", False))

    #: one kernel (ops/csrc/qkv_cache_write.hip, ops.qkv_cache_write) for
    #: what a cached decoder step does between its qkv projection and its
    #: attention kernel: the q/k/v split, CodeGen's rotary transform of q
    #: and k, q made contiguous, and the write of k and v into the bf16 or
    #: e4m3 KV cache at per-slot positions read on the device.  Taken by
    #: DecoderBlock._attn on every cached call inside
    #: ops.qkv_cache_write_ok; training and the CPU keep the torch ops.  It
    #: is what gives CodeGen per-slot positions (forward_decode,
    #: generate_graphed).  For OPT and BLOOM it moves the same bits as the
    #: torch ops; for CodeGen the rotation is done in fp32 and rounded once
    #: where apply_rotary rounds to bf16 after every op.
    #: Rule: every shape class takes the kernel, because none measured
    #: slower than the torch ops beyond the repeat-to-repeat spread
    #: (tools/qkv_cache_bench.py on one MI355X, table in docs/BENCHMARK.md,
    #: "Fused qkv split, rotary and cache write"; us per call, torch ->
    #: fused, spread <= 0.05 eager and <= 0.18 graphed).  CodeGen-16B heads,
    #: decode at batch 1-32: 124-127 -> 19.6-20.8 eager, 44-50 -> 3.2-4.4
    #: inside a captured graph; 2048-token prefill 181 -> 25 (bf16 cache),
    #: 176 -> 36 (e4m3).  OPT-13B heads, per-slot positions: 30 -> 19 eager
    #: and 11-13 -> 2.3-2.4 graphed (bf16 cache), 24 -> 19-20 eager and
    #: 5.1-5.3 -> 3.1-3.3 graphed (e4m3, against the one-launch append);
    #: prefill 52 -> 20 and 38 -> 25.  The eager figures are host time: one
    #: dispatch plus the envelope check.  End to end (serve_bench, prompt
    #: 128, batch 8, two alternating repeats): CodeGen-16B 11.52 / 11.87 ->
    #: 9.71 / 9.69 ms/token eager and 9.77 / 9.79 graphed (no graphed loop
    #: without the kernel); OPT-13B 9.16 / 9.27 -> 8.96 / 8.97 eager, 9.71 /
    #: 9.71 -> 9.10 / 9.11 graphed.
    #: "1" (default) on; ALPA_AMD_FUSED_QKV=0 restores the torch ops (and
    #: with them CodeGen's refusal of per-slot positions).
    fused_qkv_write: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_FUSED_QKV", "1"))

    #: the pass over the vocabulary that picks a decode step's next token
    #: as two kernels (ops/csrc/logits_sample.hip): ops.logits_topk gives
    #: GenerationMixin._log_probs_topk (sampling, every beam_search step)
    #: the local max, sum-exp and top-k in one read of the logits, and
    #: ops.sample_logits is sample_token at tp == 1, with temperature,
    #: top-k and top-p read per row on the device, which is what lets
    #: generate_graphed and ContinuousBatcher sample.  A GPU draw is the
    #: inverse CDF at one uniform per row, not torch.multinomial: a seed
    #: gives other tokens than with the switch off.
    #: Rule: every call inside ops.logits_topk_ok takes the kernels,
    #: because no shape class measured slower than the torch ops
    #: (tools/sampling_bench.py on one MI355X, table in docs/BENCHMARK.md,
    #: "Fused sampling"; bf16 logits, V 50272 / 51200 / 250880, batch 1-64,
    #: k 4 / 64; us per host-dispatched call, torch -> fused, spread <=
    #: 0.21).  sample_token: 207-254 -> 43-46 at V ~ 50k (4.7-5.8x),
    #: 249-492 -> 48-82 at V 250880 (5.0-7.4x).  _log_probs_topk: 89-168 ->
    #: 39-42 (2.3-4.0x) and 155-406 -> 40-77 (3.2-8.2x).  The fused figures
    #: at V ~ 50k are the host's dispatch floor, not device time.  The
    #: segment width was fixed from the register budget, not swept.
    #: Inside a captured graph and end to end (serve_bench) nothing was
    #: measured.
    #: "1" (default) on; ALPA_AMD_FUSED_SAMPLING=0 restores the torch ops
    #: (and with them greedy-only graphs and batches).
    fused_sampling: str = field(
        default_factory=lambda: os.environ.get("ALPA_AMD_FUSED_SAMPLING",
                                               "1"))

    #: bf16 dX GEMMs of the parallel linear layers read a transposed copy
    #: of the weight (its "twin", ops.weight_twin) that the fused AdamW
    #: kernel writes next to the weight: dY @ W (NN) becomes the TN GEMM
    #: the forward runs, which hipBLASLt serves 20-30 % faster
    #: (docs/BENCHMARK.md, "dX on weight twins").  Costs 2 B per linear-
    #: weight parameter.  Twins exist only where TrainState attaches them
    #: (serial/dp/tp bf16 training on the GPU; not ZeRO-2/3, the pipeline
    #: stages, fp8_gemm, or a model whose twins would take more than 1/32
    #: of the GPU's memory: AdamW.attach_weight_twins).  Off when the TrainState is
    #: created: nothing is allocated.  Turned off later: the optimizer
    #: keeps the twins current but dX reads W, so tests can run both
    #: routes in one process.  ALPA_AMD_WEIGHT_TWIN=0 turns it off
    weight_twin: bool = field(
        default_factory=lambda: _env_bool("ALPA_AMD_WEIGHT_TWIN", True))
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
