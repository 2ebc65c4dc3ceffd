"""Hand-checked MXFP4 quantizer cases, shared by the CPU and GPU tests.

Each case is one block of 32: (name, leading values, scale byte, leading
codes); the rest of the block is +0 (code 0).  Codes are sign<<3 | exp<<1 |
mant for the values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}."""
import torch

CASES = [
    ("zeros", [0.0], 127, [0]),
    # amax 5 -> floor(log2) = 2 -> E = 127, factor 1: 2.5 ties down to 2
    # (code 4), 5 ties down to 4 (code 6, the even one of 4 | 6), 3.5 ties up
    # to 4, 0.25 ties down to 0, 0.75 up to 1, 1.25 down to 1, 1.75 up to 2
    ("ties", [2.5, 5.0, -2.5, 3.5, 0.25, 0.75, 1.25, 1.75, -0.0], 127,
     [4, 6, 12, 6, 0, 2, 2, 4, 8]),
    # the same ties under a factor of 8
    ("ties_scaled", [20.0, 40.0, -20.0, 28.0], 130, [4, 6, 12, 6]),
    # amax 7.75 -> E = 127: beyond 6 saturates, 5.5 rounds up to 6
    ("saturation", [7.75, -7.5, 5.5, 6.0], 127, [7, 15, 7, 7]),
    # amax exactly 8 = 2^3 -> E = 128, factor 2: 8 -> 4, 1 -> 0.5, 3 -> 1.5
    ("power_of_two", [8.0, 1.0, -3.0, 0.5], 128, [6, 1, 11, 0]),
    # E clamps at 2: 2^-130 / 2^-125 = 2^-5 rounds to 0, 2^-126 -> 0.5
    ("clamp_low", [2.0 ** -130, -2.0 ** -126], 2, [0, 9]),
    # E clamps at 252: 3e38 / 2^125 = 7.05 saturates, 2^126 -> 2
    ("clamp_high", [3.0e38, -2.0 ** 126], 252, [7, 12]),
]


def rows():
    """(w fp32 [len(CASES), 32], scales uint8 [len(CASES), 1], codes uint8
    [len(CASES), 16] packed, even k in the low nibble)."""
    w = torch.zeros(len(CASES), 32)
    nib = torch.zeros(len(CASES), 32, dtype=torch.uint8)
    for i, (_, vals, _, codes) in enumerate(CASES):
        w[i, :len(vals)] = torch.tensor(vals)
        nib[i, :len(codes)] = torch.tensor(codes, dtype=torch.uint8)
    scales = torch.tensor([[c[2]] for c in CASES], dtype=torch.uint8)
    return w, scales, nib[:, 0::2] | (nib[:, 1::2] << 4)


def all_codes(N, K, seed=0):
    """(codes [N, K/2], scales [N, K/32]) not made by the quantizer: every
    block holds each of the 16 nibble codes twice, in an order of its own,
    and the scale byte 127 + (row + 2*block) % 3 - 1 varies with both."""
    g = torch.Generator().manual_seed(seed)
    nib = torch.stack([torch.randperm(32, generator=g) % 16
                       for _ in range(N * K // 32)]).to(torch.uint8)
    nib = nib.reshape(N, K)
    r = torch.arange(N).unsqueeze(1)
    b = torch.arange(K // 32).unsqueeze(0)
    scales = (127 + (r + 2 * b) % 3 - 1).to(torch.uint8)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous(), scales
