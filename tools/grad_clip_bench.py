"""Cost of global-norm gradient clipping on the GPT-2.6B parameter list
(389 bf16 tensors, 2.78e9 elements, fp32 moments), one MI355X:

  (a) ops.fused_adamw alone
  (b) torch.nn.utils.clip_grad_norm_ then ops.fused_adamw: what a user had
      to do before the fused path existed
  (c) ops.multi_tensor_sumsq then the clipped ops.fused_adamw

and the bandwidth of the sum of squares on its own (reduce + finalize
launches; bytes = the gradients read once).  Times are device-event times
per call, the median over ROUNDS rounds that alternate (a), (b), (c), each
round ITERS calls (10 x ITERS for the sum of squares) after warm-up.

Measured once on one MI355X (median of 5 rounds, spread under 0.1%):
  (a) 12.01 ms   (b) 19.00 ms   (c) 12.98 ms
  sum of squares alone 0.949 ms = 5.86 TB/s over 5.56 GB of gradients
so clipping costs 0.97 ms fused against 6.99 ms through clip_grad_norm_.
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from alpa_amd import ops
from alpa_amd.models.gpt import GPTModel, gpt_config

ROUNDS, ITERS, WARMUP = 5, 20, 3
MAX_NORM = 1.0


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


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = gpt_config("2.6B")
    shapes = [tuple(p.shape) for p in
              GPTModel(cfg, None, 1, torch.bfloat16, "meta").parameters()]
    g = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter(
        (0.02 * torch.randn(s, device="cuda", generator=g)).bfloat16())
        for s in shapes]
    grads0 = [(1e-3 * torch.randn(s, device="cuda", generator=g)).bfloat16()
              for s in shapes]
    for p, gr in zip(params, grads0):
        p.grad = gr.clone()
    grads = [p.grad for p in params]
    ps = [p.data for p in params]
    ms = [torch.zeros(s, device="cuda") for s in shapes]
    vs = [torch.zeros(s, device="cuda") for s in shapes]
    numel = sum(p.numel() for p in ps)
    kw = dict(lr=1e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01,
              grad_scale=1.0)

    def plain():
        ops.fused_adamw(ps, grads, ms, vs, 10, **kw)

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        ops.fused_adamw(ps, grads, ms, vs, 10, **kw)

    def fused_clip():
        sumsq = ops.multi_tensor_sumsq(grads)
        ops.fused_adamw(ps, grads, ms, vs, 10, **kw, grad_sumsq=sumsq,
                        max_grad_norm=MAX_NORM)

    def sumsq_only():
        ops.multi_tensor_sumsq(grads)

    # both routes see the same gradient norm; printed, not asserted
    norm_fused = ops.multi_tensor_sumsq(grads).sqrt().item()
    norm_torch = torch.nn.utils.clip_grad_norm_(params, float("inf")).item()
    print(f"tensors {len(ps)}  elements {numel / 1e9:.3f}e9  "
          f"grad norm fused {norm_fused:.6g}  torch {norm_torch:.6g}")

    # the sum of squares is ~10x shorter than a step: more calls per window
    cases = [("a_adamw", plain, ITERS), ("b_torch_clip_adamw", torch_clip,
                                         ITERS),
             ("c_fused_clip_adamw", fused_clip, ITERS),
             ("sumsq", sumsq_only, 10 * ITERS)]
    for _, fn, _ in cases:
        timed(fn, WARMUP)
    times = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, iters in cases:
            # (b) rescales the gradients in place: start every timing from
            # the same values
            for dst, src in zip(grads, grads0):
                dst.copy_(src)
            times[name].append(timed(fn, iters))
    for name, _, _ in cases:
        ts = times[name]
        print(f"{name:22s} median {statistics.median(ts):8.3f} ms  "
              f"min {min(ts):8.3f}  max {max(ts):8.3f}")
    t_sumsq = statistics.median(times["sumsq"])
    print(f"sumsq bandwidth {2 * numel / t_sumsq / 1e9:.2f} TB/s "
          f"({2 * numel / 1e9:.2f} GB of bf16 gradients read once)")
    a, b, c = (statistics.median(times[n]) for n, _, _ in cases[:3])
    print(f"clipping costs {b - a:.3f} ms with torch, {c - a:.3f} ms fused")


if __name__ == "__main__":
    main()
