"""Op-level cost of the producer-fused fp8 quantize at the GPT-2.6B shapes
(batch 32 x seq 1024 rows), one MI355X:

  LayerNorm [32768, 2560]:  add_layer_norm_fwd + fp8_quantize(dual)
                            against add_layer_norm_fp8
  bias+GeLU [32768, 10240]: bias_gelu_fwd + fp8_quantize(dual)
                            against bias_gelu_fp8

Times are device-event times per call, the median over ROUNDS rounds that
alternate the pair and the fused op, each round ITERS calls after warm-up.
GB/s counts the bytes each route has to move through HBM (L2 re-reads
inside a kernel are free): per element
  LayerNorm pair  2+2 read, 2 (h) + 2 (y) written, 2 (y) read, 1+1 written
  LayerNorm fused 2+2 read, 2 (h) + 1 + 1 written
  GeLU pair       2 read, 2 written, 2 read, 1+1 written
  GeLU fused      2 read, 1+1 written
The outputs of the two routes are compared byte for byte before timing.

Prints one JSON line; `--out FILE` also writes it there.

Measured once on one MI355X (spread over the rounds under 3%):
  LayerNorm pair 0.258 ms (3899 GB/s)  fused 0.224 ms (2999 GB/s)  1.15x
  GeLU pair      0.684 ms (3923 GB/s)  fused 0.402 ms (3338 GB/s)  1.70x
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from alpa_amd.ops._backend import hip_ops

ROUNDS, ITERS, WARMUP = 7, 20, 3
ROWS, HIDDEN, FFN = 32768, 2560, 10240
EPS = 1e-5


def timed(fn, iters=ITERS):
    """Mean device time of one call, in ms."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def compare(name, pair, fused, bytes_pair, bytes_fused, same):
    for a, b in same():
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    for _ in range(WARMUP):
        pair()
        fused()
    tp, tf = [], []
    for _ in range(ROUNDS):
        tp.append(timed(pair))
        tf.append(timed(fused))
    mp, mf = statistics.median(tp), statistics.median(tf)
    return {
        "pair_ms": round(mp, 4), "fused_ms": round(mf, 4),
        "pair_ms_min_max": [round(min(tp), 4), round(max(tp), 4)],
        "fused_ms_min_max": [round(min(tf), 4), round(max(tf), 4)],
        "pair_GBps": round(bytes_pair / mp / 1e6, 1),
        "fused_GBps": round(bytes_fused / mf / 1e6, 1),
        "speedup": round(mp / mf, 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = hip_ops()
    n = args.rows
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, mul=1.0, add=0.0):
        return (torch.randn(*shape, device="cuda", generator=g) * mul
                + add).bfloat16()

    scale = torch.tensor([4.0 / 448.0], device="cuda")
    result = {"rows": n, "rounds": ROUNDS, "iters": ITERS}

    a, d = rnd(n, HIDDEN), rnd(n, HIDDEN, mul=0.5)
    w, b = rnd(HIDDEN, mul=0.1, add=1.0), rnd(HIDDEN, mul=0.1)

    def ln_pair():
        h, y, mean, rstd = ext.add_layer_norm_fwd(a, d, w, b, EPS)
        return (h, mean, rstd) + tuple(ext.fp8_quantize(y, scale, True,
                                                        False))

    def ln_fused():
        return ext.add_layer_norm_fp8(a, d, w, b, EPS, scale)

    el = n * HIDDEN
    result["layer_norm"] = compare(
        "layer_norm", ln_pair, ln_fused, 12 * el, 8 * el,
        lambda: zip(ln_pair(), ln_fused()))
    del a, d

    x, gb = rnd(n, FFN), rnd(FFN, mul=0.1)

    def gelu_pair():
        return ext.fp8_quantize(ext.bias_gelu_fwd(x, gb), scale, True, False)

    def gelu_fused():
        return ext.bias_gelu_fp8(x, gb, scale)

    el = n * FFN
    result["bias_gelu"] = compare(
        "bias_gelu", gelu_pair, gelu_fused, 8 * el, 4 * el,
        lambda: zip(gelu_pair(), gelu_fused()))

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
