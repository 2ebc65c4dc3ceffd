"""Single-token decode attention on one MI355X, two routes in one process:

  (a) what a decode step took before the split-KV kernel existed:
      ext.attn_fwd with kv_lens (the prefill kernel, one workgroup per
      (batch, head)); for head_dim 256, which that route cannot mask,
      ext.attn_fwd_blocked on the cache sliced to the slot length, as
      forward_step does
  (b) ext.attn_decode (csrc/attention_decode.hip)

Shapes (heads, head_dim): (40, 128) OPT-13B, (56, 128) OPT-30B, (32, 128)
with ALiBi BLOOM-7.1B, (24, 256) CodeGen-16B; batch 1, 8, 32; slot length
128, 512, 2048; each once with Skv equal to the length and once with
Skv = 2048 of capacity and the shorter length, the graph-capture situation.

Times are device-event times per call in microseconds, the median over
ROUNDS rounds that alternate (a) and (b), each round ITERS calls after
warm-up; "spread" is the larger (max - min) / median of the two routes.  GB/s
counts what (b) has to move, from the shapes: K and V of the visible rows,
2 * B * H * len * D * 2 bytes, plus its fp32 workspace written and read once.
"%HBM" is that over the 6.3 TB/s achievable HBM rate.  Rows marked "cache"
move less than the 256 MB Infinity Cache and are repeated on the same
buffers: their rate is a cache rate, not an HBM rate.  max|a-b| is printed,
not asserted.

Measured once on one MI355X (CHUNK = 128; spread as defined above; a
timed window is 20 calls, so the short rows time well under a millisecond
of work per round and lean on the five alternating rounds):

model          H   D   B   len   Skv     a us     b us    a/b spread    GB/s  %HBM  max|a-b|
OPT-13B       40 128   1   128   128      9.4      6.4   1.47   0.02     412   6.5     0.002 cache
OPT-13B       40 128   1   128  2048     92.6     10.5   8.81   0.01     254   4.0     0.002 cache
OPT-13B       40 128   1   512   512     26.4     10.0   2.65   0.01    1068  17.0   0.00098 cache
OPT-13B       40 128   1   512  2048     92.9     12.1   7.66   0.05     879  13.9   0.00098 cache
OPT-13B       40 128   1  2048  2048    100.8     18.5   5.45   0.01    2304  36.6   0.00098 cache
OPT-13B       40 128   8   128   128     17.7      6.8   2.59   0.03    3069  48.7    0.0039 cache
OPT-13B       40 128   8   128  2048    183.7     28.3   6.49   0.03     752  11.9    0.0039 cache
OPT-13B       40 128   8   512   512     55.7     18.2   3.06   0.02    4679  74.3     0.002 cache
OPT-13B       40 128   8   512  2048    188.3     31.4   5.99   0.02    2712  43.0     0.002 cache
OPT-13B       40 128   8  2048  2048    220.3     64.6   3.41   0.03    5280  83.8   0.00098
OPT-13B       40 128  32   128   128     44.8     14.3   3.13   0.02    5860  93.0    0.0078 cache
OPT-13B       40 128  32   128  2048    464.6     86.0   5.40   0.01     991  15.7    0.0078 cache
OPT-13B       40 128  32   512   512    149.6     59.8   2.50   0.02    5699  90.5     0.002
OPT-13B       40 128  32   512  2048    484.5    112.0   4.33   0.01    3043  48.3     0.002
OPT-13B       40 128  32  2048  2048    552.9    243.9   2.27   0.01    5590  88.7   0.00098
OPT-30B       56 128   1   128   128      9.2      6.3   1.45   0.03     580   9.2     0.002 cache
OPT-30B       56 128   1   128  2048     92.5     11.2   8.27   0.01     333   5.3     0.002 cache
OPT-30B       56 128   1   512   512     26.5     10.3   2.56   0.01    1442  22.9   0.00098 cache
OPT-30B       56 128   1   512  2048     93.2     12.9   7.24   0.03    1158  18.4   0.00098 cache
OPT-30B       56 128   1  2048  2048    101.1     20.3   4.99   0.01    2945  46.7   0.00098 cache
OPT-30B       56 128   8   128   128     18.3      7.6   2.41   0.01    3871  61.4    0.0039 cache
OPT-30B       56 128   8   128  2048    185.5     36.0   5.16   0.02     829  13.2    0.0039 cache
OPT-30B       56 128   8   512   512     56.9     25.1   2.26   0.04    4748  75.4     0.002 cache
OPT-30B       56 128   8   512  2048    190.6     39.7   4.80   0.01    3006  47.7     0.002 cache
OPT-30B       56 128   8  2048  2048    222.9     91.7   2.43   0.01    5207  82.6   0.00098
OPT-30B       56 128  32   128   128     61.3     21.3   2.88   0.02    5520  87.6    0.0039 cache
OPT-30B       56 128  32   128  2048    650.2    117.2   5.55   0.01    1018  16.2    0.0039 cache
OPT-30B       56 128  32   512   512    208.0     87.6   2.37   0.02    5450  86.5     0.002
OPT-30B       56 128  32   512  2048    677.3    154.6   4.38   0.01    3086  49.0     0.002
OPT-30B       56 128  32  2048  2048    770.7    334.1   2.31   0.01    5714  90.7   0.00098
BLOOM-7.1B    32 128   1   128   128      9.6      6.3   1.51   0.01     331   5.2    0.0078 cache
BLOOM-7.1B    32 128   1   128  2048     91.9      9.9   9.32   0.08     216   3.4    0.0078 cache
BLOOM-7.1B    32 128   1   512   512     28.1     10.3   2.73   0.01     829  13.2    0.0078 cache
BLOOM-7.1B    32 128   1   512  2048     93.7     11.1   8.41   0.04     765  12.1    0.0078 cache
BLOOM-7.1B    32 128   1  2048  2048    102.6     16.1   6.36   0.01    2113  33.5    0.0078 cache
BLOOM-7.1B    32 128   8   128   128     10.3      6.5   1.58   0.03    2574  40.9     0.016 cache
BLOOM-7.1B    32 128   8   128  2048     93.6     23.9   3.91   0.04     712  11.3     0.016 cache
BLOOM-7.1B    32 128   8   512   512     32.0     16.5   1.93   0.01    4120  65.4    0.0078 cache
BLOOM-7.1B    32 128   8   512  2048     98.3     26.7   3.68   0.02    2551  40.5    0.0078 cache
BLOOM-7.1B    32 128   8  2048  2048    111.9     51.5   2.17   0.01    5293  84.0    0.0078
BLOOM-7.1B    32 128  32   128   128     38.4     12.4   3.10   0.07    5416  86.0    0.0078 cache
BLOOM-7.1B    32 128  32   128  2048    369.9     70.4   5.25   0.01     968  15.4    0.0078 cache
BLOOM-7.1B    32 128  32   512   512    117.9     44.9   2.63   0.04    6079  96.5     0.016
BLOOM-7.1B    32 128  32   512  2048    386.8     79.7   4.86   0.01    3423  54.3     0.016
BLOOM-7.1B    32 128  32  2048  2048    478.6    197.9   2.42   0.01    5512  87.5    0.0078
CodeGen-16B   24 256   1   128   128     95.8      9.4  10.20   0.34     335   5.3    0.0039 cache
CodeGen-16B   24 256   1   128  2048    104.5     13.7   7.63   0.29     233   3.7    0.0039 cache
CodeGen-16B   24 256   1   512   512     95.3     13.6   7.02   0.31     942  15.0    0.0039 cache
CodeGen-16B   24 256   1   512  2048    104.1     14.9   6.97   0.26     856  13.6    0.0039 cache
CodeGen-16B   24 256   1  2048  2048     97.1     20.6   4.70   0.31    2476  39.3   0.00098 cache
CodeGen-16B   24 256   8   128   128     95.5     10.4   9.16   0.27    2414  38.3    0.0039 cache
CodeGen-16B   24 256   8   128  2048    105.9     31.6   3.36   0.25     810  12.9    0.0039 cache
CodeGen-16B   24 256   8   512   512     96.2     21.2   4.54   0.28    4824  76.6    0.0039 cache
CodeGen-16B   24 256   8   512  2048    104.7     37.4   2.80   0.25    2733  43.4    0.0039 cache
CodeGen-16B   24 256   8  2048  2048    126.3     82.5   1.53   0.01    4955  78.6     0.002
CodeGen-16B   24 256  32   128   128     95.6     17.2   5.56   0.28    5850  92.9     0.012 cache
CodeGen-16B   24 256  32   128  2048    105.2     95.0   1.11   0.27    1077  17.1     0.012 cache
CodeGen-16B   24 256  32   512   512    119.0     78.3   1.52   0.08    5226  83.0    0.0049
CodeGen-16B   24 256  32   512  2048    282.9    131.8   2.15   0.01    3104  49.3    0.0049
CodeGen-16B   24 256  32  2048  2048    350.8    294.1   1.19   0.01    5562  88.3     0.002

(b) is faster in every row, and by more than the spread in every row but
one: CodeGen-16B, batch 32, length 128 in 2048 keys of capacity (1.11x,
spread 0.27, all of it on the hipBLASLt side).  That row has no route (a)
in the library: masking by kv_lens at head_dim 256 exists in the decode
kernel only, and route (a) there is timed on a cache sliced by hand.  Its
cost in (b) is the 15 dead chunks per (batch, head), which load nothing
but still take 6-7 ns each to dispatch.
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from alpa_amd.models.bloom import alibi_slopes
from alpa_amd.ops import DECODE_ATTN_CHUNK
from alpa_amd.ops._backend import hip_ops

ROUNDS, ITERS, WARMUP = 5, 20, 3
SHAPES = [("OPT-13B", 40, 128, False), ("OPT-30B", 56, 128, False),
          ("BLOOM-7.1B", 32, 128, True), ("CodeGen-16B", 24, 256, False)]
BATCHES = (1, 8, 32)
LENGTHS = (128, 512, 2048)
CAPACITY = 2048
HBM_BYTES_PER_S = 6.3e12
INFINITY_CACHE_BYTES = 256 * 2 ** 20


def timed(fn, iters=ITERS):
    """Mean device time of one call, in us."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    ext = hip_ops()
    print(f"{'model':12s} {'H':>3s} {'D':>3s} {'B':>3s} {'len':>5s} "
          f"{'Skv':>5s} {'a us':>8s} {'b us':>8s} {'a/b':>6s} "
          f"{'spread':>6s} {'GB/s':>7s} {'%HBM':>5s} {'max|a-b|':>9s}")
    for name, H, D, alibi in SHAPES:
        slopes = alibi_slopes(H).cuda() if alibi else None
        scale = D ** -0.5
        for B in BATCHES:
            g = torch.Generator(device="cuda").manual_seed(0)
            q = torch.randn(B, H, 1, D, device="cuda", generator=g).bfloat16()
            kcap = torch.randn(B, H, CAPACITY, D, device="cuda",
                               generator=g).bfloat16()
            vcap = torch.randn(B, H, CAPACITY, D, device="cuda",
                               generator=g).bfloat16()
            for n in LENGTHS:
                for Skv in sorted({n, CAPACITY}):
                    if Skv == CAPACITY:
                        k, v = kcap, vcap
                    else:
                        k = kcap[:, :, :Skv].contiguous()
                        v = vcap[:, :, :Skv].contiguous()
                    lens = torch.full((B,), n, dtype=torch.int32,
                                      device="cuda")

                    if D <= 128:
                        def path_a():
                            return ext.attn_fwd(q, k, v, False, scale,
                                                slopes, lens)[0]
                    else:
                        def path_a():
                            return ext.attn_fwd_blocked(
                                q, k[:, :, :n], v[:, :, :n], False, scale)[0]

                    def path_b():
                        return ext.attn_decode(q, k, v, scale, slopes,
                                               lens)[0]

                    diff = (path_a().float() - path_b().float()) \
                        .abs().max().item()
                    cases = [("a", path_a), ("b", path_b)]
                    for _, fn in cases:
                        timed(fn, WARMUP)
                    times = {c: [] for c, _ in cases}
                    for _ in range(ROUNDS):
                        for c, fn in cases:
                            times[c].append(timed(fn))
                    a = statistics.median(times["a"])
                    b = statistics.median(times["b"])
                    n_chunks = -(-Skv // DECODE_ATTN_CHUNK(D))
                    live = -(-n // DECODE_ATTN_CHUNK(D))
                    ws = 0 if n_chunks == 1 else 2 * B * H * live * (D + 2) * 4
                    moved = 2 * B * H * n * D * 2 + ws
                    rate = moved / (b * 1e-6)
                    tag = " cache" if moved < INFINITY_CACHE_BYTES else ""
                    print(f"{name:12s} {H:3d} {D:3d} {B:3d} {n:5d} {Skv:5d} "
                          f"{a:8.1f} {b:8.1f} {a / b:6.2f} "
                          f"{max(spread(times['a']), spread(times['b'])):6.2f}"
                          f" {rate / 1e9:7.0f} {100 * rate / HBM_BYTES_PER_S:5.1f}"
                          f" {diff:9.2g}{tag}")
            del q, kcap, vcap
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
