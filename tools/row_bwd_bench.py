"""The three row-kernel backward entries at the GPT-2.6B step shapes, one
MI355X:

  ln      layer_norm_bwd      [32768, 2560]
  ln_dh   add_layer_norm_bwd  [32768, 2560] with the residual gradient dh
  gelu    bias_gelu_bwd       [32768, 10240]

each timed as the autograd functions use it: dx plus the reduced vectors
(dw and db, or dbias) in bf16, the parameter dtype.  An extension that takes
out_dtype (ABI >= 9) gets it; an older one returns fp32 vectors and the
`.to(bfloat16)` casts that its callers ran are timed with it.  So the same
file, copied into an older tree, measures that tree, and two trees are
compared by running it in each.

Times are device-event times per call, the median over ROUNDS rounds that
alternate the three entries, each round ITERS calls after warm-up.  GB/s is
over the bytes an entry has to move, from the shape alone (MUST_MOVE): every
bf16 operand read once and dx written once.  The [P, F] partial round trip
and the vectors are overhead, not counted.

  python tools/row_bwd_bench.py [--save FILE]
  python tools/row_bwd_bench.py --compare OLD NEW

--save also writes the sha256 of each dx and the reduced vectors (fp32 and
bf16) of seeded inputs to FILE; --compare reads two such files (no GPU) and
reports whether the dx match bit for bit, how far the vectors differ in fp32
ulps, and how many of their bf16 roundings flip.
"""
import argparse
import hashlib
import statistics
import sys

import torch

sys.path.insert(0, ".")

ROUNDS, ITERS, WARMUP = 7, 20, 5
N, H, F = 32768, 2560, 10240
BF16 = torch.bfloat16

#: bf16 tensors of the shape that an entry reads plus the dx it writes
MUST_MOVE = {"ln": 3, "ln_dh": 4, "gelu": 3}


def must_move_bytes(name):
    return MUST_MOVE[name] * N * (F if name == "gelu" else H) * 2


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


def _entries(ext):
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g).to(BF16)

    x, dy, dh, w = rnd(N, H), rnd(N, H), rnd(N, H), rnd(H)
    xf = x.float()
    mean = xf.mean(-1)
    rstd = torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5)
    del xf
    gx, gdy, gb = rnd(N, F), rnd(N, F), rnd(F)
    takes_dtype = getattr(ext, "ABI_VERSION", 0) >= 9

    def call(entry, *args):
        if takes_dtype:
            return entry(*args, BF16)
        dx, *vecs = entry(*args)
        return (dx, *(v.to(BF16) for v in vecs))

    cases = {
        "ln": lambda: call(ext.layer_norm_bwd, dy, x, w, mean, rstd),
        "ln_dh": lambda: call(ext.add_layer_norm_bwd, dy, dh, x, w, mean,
                              rstd),
        "gelu": lambda: call(ext.bias_gelu_bwd, gdy, gx, gb),
    }
    fp32 = {
        "ln": lambda: ext.layer_norm_bwd(dy, x, w, mean, rstd),
        "ln_dh": lambda: ext.add_layer_norm_bwd(dy, dh, x, w, mean, rstd),
        "gelu": lambda: ext.bias_gelu_bwd(gdy, gx, gb),
    }
    return cases, fp32


def bench(save):
    assert torch.cuda.is_available(), "needs a GPU"
    from alpa_amd.ops._backend import hip_ops
    ext = hip_ops()
    assert ext is not None, "the HIP extension must be built"
    cases, fp32 = _entries(ext)
    for fn in cases.values():
        timed(fn, WARMUP)
    times = {name: [] for name in cases}
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            times[name].append(timed(fn))
    print(f"extension ABI {getattr(ext, 'ABI_VERSION', 0)}; median of "
          f"{ROUNDS} alternated rounds of {ITERS} calls")
    for name, ts in times.items():
        med = statistics.median(ts)
        print(f"  {name:6s} median {med:7.4f} ms  min {min(ts):7.4f}  "
              f"max {max(ts):7.4f}  {must_move_bytes(name) / med / 1e6:7.1f} "
              f"GB/s of {MUST_MOVE[name]} x [N, W] bf16")
    if save:
        record = {}
        for name in cases:
            dx, *v16 = cases[name]()
            _, *v32 = fp32[name]()
            raw = dx.view(torch.int16).cpu().numpy().tobytes()
            record[name] = dict(dx_sha256=hashlib.sha256(raw).hexdigest(),
                                fp32=[v.cpu() for v in v32],
                                bf16=[v.cpu() for v in v16])
            print(f"  {name:6s} dx sha256 {record[name]['dx_sha256'][:16]}")
        torch.save(record, save)


def compare(old_file, new_file):
    old, new = torch.load(old_file), torch.load(new_file)
    for name in old:
        a, b = old[name], new[name]
        same = a["dx_sha256"] == b["dx_sha256"]
        print(f"{name}: dx {'identical' if same else 'DIFFERS'}")
        for k, (va, vb) in enumerate(zip(a["fp32"], b["fp32"])):
            # spacing of fp32 at the larger magnitude of the pair
            mag = torch.maximum(va.abs(), vb.abs()).clamp_min(2.0 ** -126)
            ulp = torch.exp2(torch.floor(torch.log2(mag)) - 23)
            ulps = ((va.double() - vb.double()).abs() / ulp.double()).max()
            flips = (a["bf16"][k].view(torch.int16)
                     != b["bf16"][k].view(torch.int16)).sum().item()
            # a column whose terms nearly cancel is many of its own ulps off
            # at an ordinary absolute difference: print that too
            absd = (va.double() - vb.double()).abs().max().item()
            rms = va.double().pow(2).mean().sqrt().item()
            print(f"  vector {k}: max fp32 difference {ulps.item():.1f} ulp "
                  f"({absd:.3g} absolute, rms value {rms:.3g}), "
                  f"{flips} of {va.numel()} bf16 values flip")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--save", metavar="FILE")
    p.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = p.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        bench(args.save)


if __name__ == "__main__":
    main()
