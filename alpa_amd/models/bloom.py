"""BLOOM decoder family: ALiBi attention, no positional embeddings.

Capability analog of the reference's ``examples/llm_serving/model/
bloom_model.py`` (Flax BLOOM with cache).  ALiBi is computed INSIDE the
gfx950 attention kernels (ops/csrc/attention.hip: per-head slope fma on
the score tile — fwd, bwd-dq and bwd-dkv), so both training and cached
decode stay on the fused path with zero bias materialization.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from ..mesh import DeviceMesh
from .decoder import CachedDecoder, DecoderBlock, KVCache  # noqa: F401
from .gpt import LayerNorm


@dataclass
class BloomConfig:
    hidden_size: int = 1024
    num_layers: int = 24
    num_heads: int = 16
    vocab_size: int = 50304
    max_seq_len: int = 2048
    ffn_mult: int = 4
    layernorm_eps: float = 1e-5

    @property
    def head_dim(self):
        return self.hidden_size // self.num_heads


# public BLOOM ladder
BLOOM_SPECS = {
    "560M": (1024, 24, 16),
    "1.7B": (2048, 24, 16),
    "3B": (2560, 30, 32),
    "7.1B": (4096, 30, 32),
    "176B": (14336, 70, 112),
}


def bloom_config(name: str, max_seq_len: int = 2048) -> BloomConfig:
    h, l, heads = BLOOM_SPECS[name]
    return BloomConfig(hidden_size=h, num_layers=l, num_heads=heads,
                       max_seq_len=max_seq_len)


def alibi_slopes(num_heads: int) -> torch.Tensor:
    """Per-head ALiBi slopes (the BLOOM/press-et-al geometric ladder):
    for 2^k heads, slope_h = 2^(-8(h+1)/H); non-powers-of-two interleave
    the next power's odd ladder."""
    def pow2_slopes(n):
        start = 2.0 ** (-(2.0 ** -(math.log2(n) - 3)))
        return [start * (start ** i) for i in range(n)]

    if math.log2(num_heads).is_integer():
        out = pow2_slopes(num_heads)
    else:
        base = 2 ** math.floor(math.log2(num_heads))
        out = pow2_slopes(base)
        extra = pow2_slopes(2 * base)[0::2][:num_heads - base]
        out = out + extra
    return torch.tensor(out, dtype=torch.float32)


class BloomBlock(DecoderBlock):
    """Sequential ln1/ln2 residuals, GeLU MLP."""

    def __init__(self, cfg: BloomConfig, mesh, axis, dtype, device, idx,
                 init_seed):
        super().__init__(cfg, mesh, axis, dtype, device, idx, init_seed,
                         gelu=True, parallel=False)


class BloomModel(CachedDecoder):
    """TP-sharded BLOOM decoder with KV-cache generation.  Each rank's
    slopes vector covers ITS heads (the TP shard offsets into the global
    slope ladder)."""

    block_cls = BloomBlock
    max_head_dim = 128  # the kernels apply ALiBi slopes up to head_dim 128

    def __init__(self, cfg: BloomConfig, mesh: Optional[DeviceMesh] = None,
                 axis: int = 1, dtype=torch.float32, device=None,
                 init_seed: int = 0):
        super().__init__(cfg, mesh, axis, dtype, device, init_seed)
        idx = mesh.axis_index(axis) if (mesh is not None and
                                        mesh.is_member) else 0
        idx = max(idx, 0)
        slopes = alibi_slopes(cfg.num_heads)[
            idx * self.heads_per_rank:(idx + 1) * self.heads_per_rank]
        self.register_buffer("slopes", slopes.to(device=device),
                             persistent=False)
        # BLOOM normalizes the embeddings before the first block
        self.ln_emb = LayerNorm(cfg.hidden_size, cfg.layernorm_eps, dtype,
                                device)

    def _embed(self, ids, pos):
        return self.ln_emb(self.wte(ids))

    def _attn_args(self):
        return {"slopes": self.slopes}

