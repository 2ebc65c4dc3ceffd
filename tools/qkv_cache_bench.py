"""Time the fused qkv split + rotary + KV-cache write kernel
(ops.qkv_cache_write, csrc/qkv_cache_write.hip) against the torch ops it
replaces, on one MI355X.

Both sides are models.decoder.split_qkv_into_cache, what a decoder block runs
between its qkv projection and its attention call, with
global_config.fused_qkv_write on and off.  Shapes: CodeGen-16B heads (h 24,
d 256, rotary 64, bf16 tables) and OPT-13B heads (h 40, d 128, no rotary);
decode at batch 1, 8, 32 and one 2048-token prefill; bf16 and e4m3 caches.
OPT decodes at per-slot device positions; CodeGen at one int position, the
only form its torch path has, and the fused path alone is also timed at
per-slot positions ("slots").

Every figure is the time per call in microseconds from device events around
a window of --iters calls (well above a millisecond), the two paths
alternating window by window, median of --repeats windows after a warm-up
window; spread = (max - min) / median over the repeats.  "eager" is
host-dispatched calls back to back, "graph" the replay of a captured graph of
20 calls (decode only).  Prints a markdown table and one JSON line.

  python tools/qkv_cache_bench.py [--iters 300] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
from alpa_amd.global_env import global_config
from alpa_amd.models.codegen import apply_rotary, rotary_tables
from alpa_amd.models.decoder import split_qkv_into_cache

FAMILIES = {"codegen16b": (24, 256, 64), "opt13b": (40, 128, None)}
CAP = 4096
GRAPH_CALLS = 20


def make_case(family, B, S, fp8, slots):
    h, d, rd = FAMILIES[family]
    dev = "cuda"
    qkv = torch.randn(B, S, 3 * h * d, device=dev).bfloat16().view(
        B, S, h, 3, d)
    if fp8:
        ck, cv = ((torch.zeros(B, h, CAP, d, dtype=torch.uint8, device=dev)
                   .view(torch.float8_e4m3fn),
                   torch.zeros(B, h, CAP, device=dev)) for _ in range(2))
    else:
        ck, cv = (torch.zeros(B, h, CAP, d, dtype=torch.bfloat16, device=dev)
                  for _ in range(2))
    if S > 1:
        pos = 0
    elif slots:
        pos = 1024 + 7 * torch.arange(B, device=dev)
    else:
        pos = 1024
    rotate = rotary = None
    if rd is not None:
        sin, cos = rotary_tables(rd, CAP, torch.bfloat16, dev)
        rotary = (sin, cos, rd)

        def rotate(x, p):
            return apply_rotary(x, sin, cos, p, rd)

    def call():
        return split_qkv_into_cache(qkv, ck, cv, pos, rotate, rotary)

    return call


def window(fn, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters       # us per call


def graphed(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            call()
    return g.replay


@torch.no_grad()
def measure(call, paths, iters, repeats, graph):
    """{path: (median us, spread)} of `call` under each switch value."""
    fns = {}
    for path in paths:
        global_config.fused_qkv_write = path
        fns[path] = graphed(call) if graph else call
    per = GRAPH_CALLS if graph else 1
    n = max(iters // per, 10)
    times = {p: [] for p in paths}
    for rep in range(repeats + 1):                      # window 0 warms up
        for path in paths:
            global_config.fused_qkv_write = path
            t = window(fns[path], n) / per
            if rep:
                times[path].append(t)
    global_config.fused_qkv_write = "1"
    return {p: (statistics.median(t), (max(t) - min(t)) /
                statistics.median(t)) for p, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    rows = []
    for family in FAMILIES:
        for fp8 in (False, True):
            shapes = [(1, 1), (8, 1), (32, 1), (1, 2048)]
            for B, S in shapes:
                # the torch path of CodeGen has no per-slot positions
                slots = S == 1 and FAMILIES[family][2] is None
                for graph in ((False, True) if S == 1 else (False,)):
                    iters = args.iters if S == 1 else max(args.iters // 6, 20)
                    r = measure(make_case(family, B, S, fp8, slots),
                                ("0", "1"), iters, args.repeats, graph)
                    row = dict(family=family, cache="e4m3" if fp8 else "bf16",
                               B=B, S=S, pos="slots" if slots else "int",
                               mode="graph" if graph else "eager",
                               torch_us=r["0"][0], torch_spread=r["0"][1],
                               fused_us=r["1"][0], fused_spread=r["1"][1])
                    if S == 1 and not slots:
                        f = measure(make_case(family, B, S, fp8, True),
                                    ("1",), iters, args.repeats, graph)
                        row["fused_slots_us"] = f["1"][0]
                    rows.append(row)
    print("| heads | cache | B | S | pos | mode | torch us | fused us | "
          "ratio | spread torch / fused | fused at slots us |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        extra = f"{r['fused_slots_us']:.1f}" if "fused_slots_us" in r else "-"
        print(f"| {r['family']} | {r['cache']} | {r['B']} | {r['S']} | "
              f"{r['pos']} | {r['mode']} | {r['torch_us']:.1f} | "
              f"{r['fused_us']:.1f} | {r['torch_us'] / r['fused_us']:.2f}x | "
              f"{r['torch_spread']:.2f} / {r['fused_spread']:.2f} | {extra} |")
    print(json.dumps({"bench": "qkv_cache_write", "iters": args.iters,
                      "repeats": args.repeats, "rows": rows}))


if __name__ == "__main__":
    main()
