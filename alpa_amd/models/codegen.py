"""CodeGen decoder family (GPT-J architecture) with rotary positions.

Capability analog of the reference's ``examples/llm_serving/model/
codegen_model.py`` (Flax CodeGen with cache).  GPT-J-style blocks:
ONE LayerNorm feeding attention AND the MLP in parallel
(x + attn(ln(x)) + mlp(ln(x))), rotary embedding applied to the first
``rotary_dim`` dims of every head (interleaved/"rotate_every_two"
convention).  Rotary is an elementwise pre-transform of q/k, so the
unmodified gfx950 flash-attention kernel serves both prefill and cached
decode; generation (greedy + beam) comes from GenerationMixin.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ..mesh import DeviceMesh
from .decoder import CachedDecoder, DecoderBlock, KVCache  # noqa: F401


@dataclass
class CodeGenConfig:
    hidden_size: int = 1024
    num_layers: int = 20
    num_heads: int = 16
    vocab_size: int = 51200
    max_seq_len: int = 2048
    rotary_dim: int = 32
    ffn_mult: int = 4
    layernorm_eps: float = 1e-5

    @property
    def head_dim(self):
        return self.hidden_size // self.num_heads


# public CodeGen ladder (350M/2B/6B/16B)
CODEGEN_SPECS = {
    "350M": (1024, 20, 16),
    "2B": (2560, 32, 32),
    "6B": (4096, 33, 16),
    "16B": (6144, 34, 24),
}


def codegen_config(name: str, max_seq_len: int = 2048) -> CodeGenConfig:
    h, l, heads = CODEGEN_SPECS[name]
    return CodeGenConfig(hidden_size=h, num_layers=l, num_heads=heads,
                         max_seq_len=max_seq_len)


def rotary_tables(rotary_dim: int, max_len: int, dtype, device):
    """(sin, cos) tables [max_len, rotary_dim//2] — GPT-J inv_freq."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, rotary_dim, 2,
                                          dtype=torch.float32) / rotary_dim))
    t = torch.arange(max_len, dtype=torch.float32)
    freqs = torch.outer(t, inv)
    return (freqs.sin().to(dtype=dtype, device=device),
            freqs.cos().to(dtype=dtype, device=device))


def apply_rotary(x: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor,
                 pos: int, rotary_dim: int) -> torch.Tensor:
    """x [B, h, S, d]: rotate the first rotary_dim dims, interleaved pairs
    (GPT-J "rotate_every_two"); positions pos..pos+S-1."""
    B, H, S, D = x.shape
    r = x[..., :rotary_dim].view(B, H, S, rotary_dim // 2, 2)
    x1, x2 = r[..., 0], r[..., 1]
    s = sin[pos:pos + S].view(1, 1, S, -1).to(x.dtype)
    c = cos[pos:pos + S].view(1, 1, S, -1).to(x.dtype)
    rot = torch.stack([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)
    return torch.cat([rot.flatten(-2), x[..., rotary_dim:]], dim=-1)


class CodeGenBlock(DecoderBlock):
    """Parallel-residual block: x + attn(ln x) + mlp(ln x) (GPT-J)."""

    def __init__(self, cfg: CodeGenConfig, mesh, axis, dtype, device, idx,
                 init_seed):
        super().__init__(cfg, mesh, axis, dtype, device, idx, init_seed,
                         gelu=True, parallel=True)


class CodeGenModel(CachedDecoder):
    """TP-sharded CodeGen decoder with KV-cache generation."""

    block_cls = CodeGenBlock

    def __init__(self, cfg: CodeGenConfig, mesh: Optional[DeviceMesh] = None,
                 axis: int = 1, dtype=torch.float32, device=None,
                 init_seed: int = 0):
        super().__init__(cfg, mesh, axis, dtype, device, init_seed)
        sin, cos = rotary_tables(cfg.rotary_dim, cfg.max_seq_len, dtype,
                                 device)
        self.register_buffer("rot_sin", sin, persistent=False)
        self.register_buffer("rot_cos", cos, persistent=False)

    def _embed(self, ids, pos):
        return self.wte(ids)

    def _rotate(self, x, pos):
        if not isinstance(pos, int):
            raise NotImplementedError(
                "CodeGen rotary takes one int position for the whole batch; "
                "per-slot positions (forward_decode, continuous batching) "
                "are not implemented")
        return apply_rotary(x, self.rot_sin, self.rot_cos, pos,
                            self.cfg.rotary_dim)

    def _attn_args(self):
        return {"rotate": self._rotate}

