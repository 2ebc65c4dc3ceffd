"""Device-event times of the GPT-2.6B step GEMMs by operand layout, and of the
AdamW step with and without weight twins.

For each linear (qkv, out, fc1, fc2, LM head) at 32768 tokens:
  - dX as it runs on the weight, dY @ W (NN), against the same product on a
    pre-transposed copy, dY @ Wt.t() (TN, the forward's layout);
  - dW as it runs, dY.t() @ x (NT), against TN with both operands
    pre-transposed, and what x.t().contiguous() costs, so that the dW
    question can be decided from numbers;
and the multi-tensor AdamW over the 2.6B linear weights: flat, with twins,
and flat plus a plain w.t().contiguous() over the same weights.

The two arms of every comparison alternate, iteration by iteration, after a
warm-up; the figure is the median.  Run with the shipped TunableOp file
loaded, as bench.py does:  python tools/gemm_layout_probe.py [--iters 30]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _tunableop():
    base = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "alpa_amd", "ops", "tuned",
        "tunableop_gfx950_.csv")
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", base)


_tunableop()

import torch  # noqa: E402


def alternate(arms, iters, warmup=5):
    """arms: {name: fn}.  Median device-event ms of each, the arms taking
    turns within every iteration."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(iters):
        for k, fn in arms.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v))
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--hidden", type=int, default=2560)
    ap.add_argument("--vocab", type=int, default=51200)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--skip-adamw", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    from alpa_amd import ops

    bf16, dev = torch.bfloat16, "cuda"
    M, H = args.tokens, args.hidden
    linears = [("qkv", 3 * H, H), ("out", H, H), ("fc1", 4 * H, H),
               ("fc2", H, 4 * H), ("lm_head", args.vocab, H)]
    rows = []
    for name, out_f, in_f in linears:
        w = torch.randn(out_f, in_f, device=dev).to(bf16)
        wt = w.t().contiguous()
        x = torch.randn(M, in_f, device=dev).to(bf16)
        dy = torch.randn(M, out_f, device=dev).to(bf16)
        r = alternate({"dx_nn": lambda: dy @ w,
                       "dx_tn": lambda: dy @ wt.t()}, args.iters)
        flops = 2.0 * M * out_f * in_f
        row = {"linear": name, "out": out_f, "in": in_f}
        for k, (med, lo, hi) in r.items():
            row[k + "_ms"] = round(med, 4)
            row[k + "_spread_ms"] = round(hi - lo, 4)
            row[k + "_pflops"] = round(flops / med / 1e12, 3)
        xt, dyt = x.t().contiguous(), dy.t().contiguous()
        r = alternate({"dw_nt": lambda: dy.t() @ x,
                       "dw_tn": lambda: dyt @ xt.t(),
                       "x_t_contiguous": lambda: x.t().contiguous()},
                      args.iters)
        for k, (med, lo, hi) in r.items():
            row[k + "_ms"] = round(med, 4)
            row[k + "_spread_ms"] = round(hi - lo, 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del w, wt, x, dy, xt, dyt
    if args.skip_adamw:
        return

    # AdamW over the linear weights of the whole model (no LM head: it has
    # no twin), zero gradients so the weights stay put over many steps
    shapes = [(o, i) for _, o, i in linears[:4]] * args.layers
    p = [torch.randn(s, device=dev).to(bf16) for s in shapes]
    g = [torch.zeros_like(t) for t in p]
    m = [torch.zeros(s, device=dev) for s in shapes]
    v = [torch.zeros(s, device=dev) for s in shapes]
    twins = [t.t().contiguous() for t in p]
    hyper = dict(lr=1e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01)

    def flat():
        ops.fused_adamw(p, g, m, v, 1, **hyper)

    def twinned():
        ops.fused_adamw(p, g, m, v, 1, twins=twins, **hyper)

    def flat_plus_transpose():
        flat()
        for t, w in zip(twins, p):
            t.copy_(w.t())

    r = alternate({"adamw_flat": flat, "adamw_twins": twinned,
                   "adamw_flat_plus_transpose": flat_plus_transpose},
                  args.iters)
    n = sum(t.numel() for t in p)
    row = {"adamw_params": n}
    for k, (med, lo, hi) in r.items():
        row[k + "_ms"] = round(med, 4)
        row[k + "_spread_ms"] = round(hi - lo, 4)
    row["adamw_flat_tbps"] = round(22 * n / r["adamw_flat"][0] / 1e9, 3)
    row["adamw_twins_tbps"] = round(24 * n / r["adamw_twins"][0] / 1e9, 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
