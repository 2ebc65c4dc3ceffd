"""Forward + backward of the loss over one vocab shard, one MI355X:

  (a) parallel.layers._VocabParallelCrossEntropy, the torch path that
      vocab-sharded logits took before the shard kernels existed
  (b) parallel.layers.fused_vocab_parallel_cross_entropy: the partial
      forward kernel, the [N]-sized combine, the shard backward kernel

both on a 1x1 mesh, where every collective is a no-op, so this times the
local work of one tensor-parallel rank and none of the communication.
Shapes (N, Vs): 8192 tokens by the tp = 2 and tp = 8 shards of the 51200
vocab.  Times are device-event times per forward+backward, the median over
ROUNDS rounds that alternate (a) and (b), each round ITERS calls after
warm-up.  Peak memory is torch.cuda.max_memory_allocated over one
forward+backward, less what was allocated before it (logits, targets,
dloss).  Bytes/s counts what the fused path has to move, computed from the
shape: the bf16 shard read twice and written once.

Measured once on one MI355X (median of 5 rounds, spread under 4%):
  (8192, 25600)  (a) 2.362 ms, 2400 MiB   (b) 0.280 ms, 400 MiB, 4.49 TB/s
  (8192,  6400)  (a) 0.626 ms,  600 MiB   (b) 0.084 ms, 100 MiB, 3.74 TB/s
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import alpa_amd as aa
from alpa_amd.parallel.layers import (_VocabParallelCrossEntropy,
                                      fused_vocab_parallel_cross_entropy)

ROUNDS, ITERS, WARMUP = 5, 20, 3
SHAPES = [(8192, 25600), (8192, 6400)]


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


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    mesh = aa.DeviceMesh([0], (1, 1))
    for N, Vs in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = torch.randn(N, Vs, device="cuda", generator=g) \
            .bfloat16().requires_grad_()
        targets = torch.randint(0, Vs, (N,), device="cuda", generator=g)
        dloss = torch.full((N,), 1.0 / N, device="cuda")

        def torch_path():
            loss = _VocabParallelCrossEntropy.apply(logits, targets, mesh, 1,
                                                    0)
            return loss, torch.autograd.grad(loss, logits, dloss)[0]

        def fused_path():
            loss = fused_vocab_parallel_cross_entropy(logits, targets, mesh,
                                                      1, 0)
            return loss, torch.autograd.grad(loss, logits, dloss)[0]

        # both routes compute the same thing; printed, not asserted
        (la, ga), (lb, gb) = torch_path(), fused_path()
        print(f"N={N} Vs={Vs}: max |loss a - b| "
              f"{(la - lb).abs().max().item():.3g}  max |grad a - b| "
              f"{(ga.float() - gb.float()).abs().max().item():.3g}")
        del la, ga, lb, gb

        cases = [("a_torch", torch_path), ("b_fused", fused_path)]
        for _, fn in cases:
            timed(fn, WARMUP)
        times = {name: [] for name, _ in cases}
        for _ in range(ROUNDS):
            for name, fn in cases:
                times[name].append(timed(fn))
        shard_bytes = 3 * N * Vs * 2
        for name, fn in cases:
            ts = times[name]
            med = statistics.median(ts)
            print(f"  {name:8s} median {med:8.3f} ms  min {min(ts):8.3f}  "
                  f"max {max(ts):8.3f}  peak extra memory "
                  f"{peak_extra_bytes(fn) / 2**20:8.1f} MiB  "
                  f"{shard_bytes / med / 1e9:6.2f} TB/s of 2 reads + 1 write")
        a, b = (statistics.median(times[n]) for n, _ in cases)
        print(f"  fused is {a / b:.2f}x the torch path")


if __name__ == "__main__":
    main()
