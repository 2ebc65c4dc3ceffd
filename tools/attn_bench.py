"""Isolated attention kernel microbenchmark (bench shapes).

Usage: python tools/attn_bench.py [--iters 20] [--packed]
Prints per-kernel time + effective TFLOPS for fwd / bwd on the GPT-2.6B
bench shape (B=8, h=32, S=1024, D=80).

--packed times the forward alone the way the flagship model calls it:
attn_fwd_out on the strided q/k/v views of one packed qkv buffer
[B, S, h*3*D], writing o as a [B, S, h*D] activation, at B=32 unless --B
is given.
"""
import argparse
import math
import sys
import time

import torch

import os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
from alpa_amd.ops._backend import hip_ops


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def packed_fwd(ext, B, H, S, D, iters):
    from alpa_amd.ops import _qkv_views
    qkv = torch.randn(B, S, H * 3 * D, device="cuda", dtype=torch.bfloat16)
    q, k, v = _qkv_views(qkv, H)
    o = torch.empty(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    o_view = o.permute(0, 2, 1, 3)
    lse = torch.empty(B, H, S, device="cuda", dtype=torch.float32)
    scale = 1.0 / math.sqrt(D)
    flops = 4 * B * H * S * S * D * 0.5  # causal
    t = timeit(lambda: ext.attn_fwd_out(q, k, v, o_view, lse, True, scale),
               iters)
    print(f"fwd packed B={B}:  {t*1e6:8.1f} us  {flops/t/1e12:7.1f} TF")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--B", type=int, default=None,
                   help="batch (default 8, or 32 with --packed)")
    p.add_argument("--packed", action="store_true",
                   help="forward only, through attn_fwd_out on packed-qkv "
                        "strided views")
    p.add_argument("--H", type=int, default=32)
    p.add_argument("--S", type=int, default=1024)
    p.add_argument("--D", type=int, default=80)
    args = p.parse_args()
    ext = hip_ops()
    B = args.B if args.B is not None else (32 if args.packed else 8)
    H, S, D = args.H, args.S, args.D
    torch.manual_seed(0)
    if args.packed:
        packed_fwd(ext, B, H, S, D, args.iters)
        return
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    scale = 1.0 / math.sqrt(D)

    fwd_flops = 4 * B * H * S * S * D * 0.5  # causal
    t = timeit(lambda: ext.attn_fwd(q, k, v, True, scale), args.iters)
    print(f"fwd:  {t*1e6:8.1f} us  {fwd_flops/t/1e12:7.1f} TF")

    o, lse = ext.attn_fwd(q, k, v, True, scale)
    do = torch.randn_like(o)
    lse3 = lse.view(B, H, S)
    bwd_flops = 10 * B * H * S * S * D * 0.5
    t = timeit(lambda: ext.attn_bwd(do, q, k, v, o, lse3, True, scale),
               args.iters)
    print(f"bwd:  {t*1e6:8.1f} us  {bwd_flops/t/1e12:7.1f} TF")


if __name__ == "__main__":
    main()
