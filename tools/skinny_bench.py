"""Numerics + bandwidth of the skinny decode kernels vs torch.matmul at
decode shapes: the dot2 GEMV (csrc/skinny_gemm.hip) and, for 9..64 tokens
inside its envelope, the MFMA skinny GEMM (csrc/skinny_mfma.hip) as a third
column.  After the bf16 and e4m3 rows come the MXFP4 rows (fp4:
csrc/skinny_fp4.hip up to 8 tokens, csrc/skinny_mfma_fp4.hip for 9..64,
against the same library bf16 GEMM; rel is against the dequantized weights).
Every column is the time of one whole call (all its launches).
SKINNY_SWEEP=1 sweeps the legal splits of both kernels, SKINNY_REPEAT=n
prints the whole table n times (the spread between the copies is the
run-to-run noise); HBM bandwidth is the bound of these GEMMs, so the floor
is weight bytes / SKINNY_PEAK_TBS (default 8 TB/s, the MI355X HBM peak)."""
import os
import sys
import time

import torch

sys.path.insert(0, ".")
from alpa_amd.ops import (_skinny_legal_splits, _skinny_mfma_legal_splits,
                          _skinny_mfma_mt, _skinny_mfma_splits, _skinny_mt,
                          _skinny_splits, mxfp4_dequantize, mxfp4_pack,
                          mxfp4_quantize)
from alpa_amd.ops._backend import hip_ops

PEAK_TBS = float(os.environ.get("SKINNY_PEAK_TBS", "8.0"))


def bench(fn, iters=300):
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def run(M, N, K, fp8):
    x = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") * 0.05).to(torch.bfloat16)
    if fp8:
        amax = w.abs().amax().float().clamp_min(1e-12)
        scale = (amax / 448.0).reshape(1)
        q = (w.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
        wp = q.view(torch.uint8).view(N, K // 8, 8).permute(1, 0, 2) \
            .contiguous()
        wref = (q.float() * scale).to(torch.bfloat16)
    else:
        scale = None
        wp = w.view(N, K // 8, 8).permute(1, 0, 2).contiguous()
        wref = w
    s = _skinny_splits(N, K, M)
    sweep = os.environ.get("SKINNY_SWEEP") == "1"
    y = hip_ops().skinny_gemm(wp, x, scale, None, N, K, s)
    ref = x.float() @ wref.float().t()
    rel = (y - ref).abs().mean() / ref.abs().mean().clamp_min(1e-9)

    t_k = bench(lambda: hip_ops().skinny_gemm(wp, x, scale, None, N, K, s))
    if sweep:
        q = K // 64
        MT = 4
        while MT < M:
            MT *= 2
        for s2 in [d for d in range(1, q + 1) if q % d == 0
                   and (K // 8 // d) * 16 * MT <= 65536]:
            t2 = bench(lambda: hip_ops().skinny_gemm(wp, x, scale, None, N, K,
                                                     s2), 100)
            if t2 < t_k:
                t_k, s = t2, s2
    t_t = bench(lambda: x @ w.t())
    bytes_w = N * K * (1 if fp8 else 2)
    line = (f"M={M:3d} N={N:6d} K={K:6d} {'fp8' if fp8 else 'bf16'} "
            f"splits={s:2d}: rel={rel.item():.4f}  kernel {t_k:7.1f} us "
            f"({bytes_w / t_k / 1e6:5.2f} TB/s)  torch {t_t:7.1f} us  "
            f"speedup {t_t / t_k:4.2f}x")
    sm = _skinny_mfma_splits(N, K, M)
    if sm is not None:
        def mfma(c):
            return hip_ops().skinny_gemm_mfma(wp, x, scale, None, N, K, c)
        rel_m = (mfma(sm) - ref).abs().mean() / ref.abs().mean() \
            .clamp_min(1e-9)
        rule, t_m = sm, bench(lambda: mfma(sm))
        t_rule = t_m
        if sweep:
            for s2 in _skinny_mfma_legal_splits(K, _skinny_mfma_mt(M)):
                t2 = bench(lambda: mfma(s2), 100)
                if t2 < t_m:
                    t_m, sm = t2, s2
        floor = bytes_w / PEAK_TBS / 1e6
        line += (f"  |  mfma splits={sm:2d} (rule {rule:2d}: {t_rule:6.1f} us)"
                 f" rel={rel_m.item():.4f} {t_m:7.1f} us "
                 f"({bytes_w / t_m / 1e6:5.2f} TB/s, {floor / t_m:4.0%} of "
                 f"the HBM floor)  vs torch {t_t / t_m:4.2f}x  "
                 f"vs dot2 {t_k / t_m:4.2f}x")
    print(line, flush=True)


def run_fp4(M, N, K):
    """One MXFP4 row: the kernel that serves M tokens, at the rule's split
    (and, under SKINNY_SWEEP=1, at the best legal one)."""
    x = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") * 0.05).to(torch.bfloat16)
    codes, scales = mxfp4_quantize(w)
    wq, sq = mxfp4_pack(codes, scales)
    ref = x.float() @ mxfp4_dequantize(codes, scales).float().t()
    if M <= 8:
        name, gemm = "dot2", hip_ops().skinny_gemm_fp4
        s = _skinny_splits(N, K, M, True)
        legal = _skinny_legal_splits(K, _skinny_mt(M), True)
    else:
        name, gemm = "mfma", hip_ops().skinny_gemm_mfma_fp4
        s = _skinny_mfma_splits(N, K, M)
        legal = _skinny_mfma_legal_splits(K, _skinny_mfma_mt(M))
    if s is None:
        return

    def fp4(c):
        return gemm(wq, sq, x, None, N, K, c)
    rel = (fp4(s) - ref).abs().mean() / ref.abs().mean().clamp_min(1e-9)
    rule, t_k = s, bench(lambda: fp4(s))
    t_rule = t_k
    if os.environ.get("SKINNY_SWEEP") == "1":
        for s2 in legal:
            t2 = bench(lambda: fp4(s2), 100)
            if t2 < t_k:
                t_k, s = t2, s2
    t_t = bench(lambda: x @ w.t())
    bytes_w = N * K // 2 + N * K // 32
    floor = bytes_w / PEAK_TBS / 1e6
    print(f"M={M:3d} N={N:6d} K={K:6d} fp4  {name} splits={s:2d} (rule "
          f"{rule:2d}: {t_rule:6.1f} us) rel={rel.item():.4f} {t_k:7.1f} us "
          f"({bytes_w / t_k / 1e6:5.2f} TB/s, {floor / t_k:4.0%} of the HBM "
          f"floor)  torch {t_t:7.1f} us  vs torch {t_t / t_k:4.2f}x",
          flush=True)


_shapes = os.environ.get("SKINNY_SHAPES")
SHAPES = ([tuple(map(int, t.split("x"))) for t in _shapes.split(",")]
          if _shapes else [(5120, 5120), (15360, 5120), (20480, 5120),
                           (5120, 20480)])
MS = tuple(int(m) for m in
           os.environ.get("SKINNY_MS", "4,16,64").split(","))
for rep in range(int(os.environ.get("SKINNY_REPEAT", "1"))):
    for fp8 in (False, True):
        for (N, K) in SHAPES:
            for M in MS:
                run(M, N, K, fp8)
    for (N, K) in SHAPES:
        for M in MS:
            run_fp4(M, N, K)
