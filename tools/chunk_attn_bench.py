"""Sq query rows over a KV cache on one MI355X, two routes in one process:

  (a) the only thing the library could do for this input before the chunk
      kernel: Sq calls of ext.attn_decode (ext.attn_decode_fp8 over the e4m3
      cache), row i with lengths len - Sq + i + 1
  (b) ext.attn_chunk / ext.attn_chunk_fp8 (csrc/attention_chunk.hip), one
      call

Shapes: (heads, head_dim) (32, 128) and (24, 256); Sq 4, 16, 64; cache
length 512, 2048 (Skv equal to it); batch 1, 8; both caches.

Times are device-event times per call in microseconds, the median over
ROUNDS rounds that alternate (a) and (b), each round ITERS calls after
warm-up; "spread" is the larger (max - min) / median of the two routes.
"floor" is the time to stream the visible cache bytes once (K and V rows,
and their scales for e4m3) at the 6.3 TB/s achievable HBM rate: every row
here moves less than the 256 MB Infinity Cache and repeats on the same
buffers, so the floor is a yardstick, not a bound that was hit.  max|a-b| is
printed, not asserted.  The table of one run is in docs/BENCHMARK.md, "Chunk
attention".
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from alpa_amd.ops._backend import hip_ops

ROUNDS, ITERS, WARMUP = 5, 20, 3
SHAPES = [(32, 128), (24, 256)]
HBM_BYTES_PER_US = 6.3e6


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
    print(f"{'cache':5s} {'H':>3s} {'D':>3s} {'B':>2s} {'len':>5s} {'Sq':>3s} "
          f"{'a us':>8s} {'b us':>8s} {'a/b':>6s} {'spread':>6s} "
          f"{'floor us':>8s} {'b/floor':>7s} {'max|a-b|':>9s}")
    for H, D in SHAPES:
        scale = D ** -0.5
        for B in (1, 8):
            for n in (512, 2048):
                g = torch.Generator(device="cuda").manual_seed(0)
                k, v = (torch.randn(B, H, n, D, device="cuda",
                                    generator=g).bfloat16() for _ in "kv")
                c8 = [torch.zeros(B, H, n, D, dtype=torch.uint8, device="cuda"
                                  ).view(torch.float8_e4m3fn),
                      torch.zeros(B, H, n, device="cuda")]
                c8 += [t.clone() for t in c8]
                ext.kv_cache_append(k, v, *c8, 0, None)
                for cache, kv, dec, chunk, row_bytes in (
                        ("bf16", [k, v], ext.attn_decode, ext.attn_chunk,
                         2 * D),
                        ("e4m3", c8, ext.attn_decode_fp8, ext.attn_chunk_fp8,
                         D + 4)):
                    for Sq in (4, 16, 64):
                        q = torch.randn(B, H, Sq, D, device="cuda",
                                        generator=g).bfloat16()
                        rows = [q[:, :, i:i + 1] for i in range(Sq)]
                        lens = [torch.full((B,), n - Sq + i + 1,
                                           dtype=torch.int32, device="cuda")
                                for i in range(Sq)]

                        def path_a():
                            return [dec(rows[i], *kv, scale, None, lens[i])[0]
                                    for i in range(Sq)]

                        def path_b():
                            return chunk(q, *kv, scale, None, None)[0]

                        diff = (torch.cat(path_a(), 2).float() -
                                path_b().float()).abs().max().item()
                        cases = [("a", path_a), ("b", path_b)]
                        for _, fn in cases:
                            timed(fn, WARMUP)
                        times = {c: [] for c, _ in cases}
                        for _ in range(ROUNDS):
                            for c, fn in cases:
                                times[c].append(timed(fn))
                        a, b = (statistics.median(times[x]) for x in "ab")
                        floor = 2 * B * H * n * row_bytes / HBM_BYTES_PER_US
                        print(f"{cache:5s} {H:3d} {D:3d} {B:2d} {n:5d} "
                              f"{Sq:3d} {a:8.1f} {b:8.1f} {a / b:6.2f} "
                              f"{max(spread(t) for t in times.values()):6.2f}"
                              f" {floor:8.2f} {b / floor:7.1f} {diff:9.2g}",
                              flush=True)


if __name__ == "__main__":
    main()
