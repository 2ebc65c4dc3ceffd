"""Time the top-k log-prob and sampling kernels (ops.logits_topk /
ops.sample_logits, csrc/logits_sample.hip) against the torch ops they
replace, on one MI355X.

Both sides are GenerationMixin calls at tp == 1 with
global_config.fused_sampling off and on: "sample" is sample_token
(_log_probs_topk plus the draw: temperature 0.8, top_p 0.9, top_k = k),
"topk" is _log_probs_topk(logits, k) alone, one beam-search step.  Shapes:
bf16 logits [B, V], V in 50272 (OPT), 51200 (GPT ladder), 250880 (BLOOM), B
in 1, 8, 32, 64, k in 4, 64.

Every figure is the time per call in microseconds from device events around
a window of --iters host-dispatched calls (well above a millisecond), the two
paths alternating window by window, median of --repeats windows after a
warm-up window; spread = (max - min) / median over the repeats.  Prints a
markdown table and one JSON line.

  python tools/sampling_bench.py [--iters 200] [--repeats 5]
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
from alpa_amd.models.generation import GenerationMixin


class _Head(GenerationMixin):
    mesh = None
    axis = 1


def window(fn, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters       # us per call


@torch.no_grad()
def measure(call, iters, repeats):
    """{switch: (median us, spread)} of `call` with the switch off and on."""
    times = {"0": [], "1": []}
    for rep in range(repeats + 1):                      # window 0 warms up
        for path in times:
            global_config.fused_sampling = path
            t = window(call, iters)
            if rep:
                times[path].append(t)
    global_config.fused_sampling = "1"
    return {p: (statistics.median(t), (max(t) - min(t)) /
                statistics.median(t)) for p, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    head = _Head()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for V in (50272, 51200, 250880):
        for B in (1, 8, 32, 64):
            logits = (3 * torch.randn(B, V, device="cuda")).bfloat16()
            for k in (4, 64):
                calls = {
                    "sample": lambda: head.sample_token(logits, 0.8, k, 0.9,
                                                        gen),
                    "topk": lambda: head._log_probs_topk(logits, k)}
                for what, call in calls.items():
                    r = measure(call, args.iters, args.repeats)
                    rows.append(dict(V=V, B=B, k=k, what=what,
                                     torch_us=r["0"][0],
                                     torch_spread=r["0"][1],
                                     fused_us=r["1"][0],
                                     fused_spread=r["1"][1]))
    print("| V | B | k | call | torch us | fused us | ratio | "
          "spread torch / fused |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['V']} | {r['B']} | {r['k']} | {r['what']} | "
              f"{r['torch_us']:.1f} | {r['fused_us']:.1f} | "
              f"{r['torch_us'] / r['fused_us']:.2f}x | "
              f"{r['torch_spread']:.2f} / {r['fused_spread']:.2f} |")
    print(json.dumps({"bench": "fused_sampling", "iters": args.iters,
                      "repeats": args.repeats, "rows": rows}))


if __name__ == "__main__":
    main()
