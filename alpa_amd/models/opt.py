"""OPT decoder family with KV-cache generation (serving).

Capability analog of the reference's llm_serving stack
(``examples/llm_serving/model/wrapper.py:501`` get_model builds pipeshard
inference executables with the KV cache as DistributedArrays;
``model/opt_model.py`` is the Flax OPT with cache).  Here: TP-sharded OPT
modules over a DeviceMesh axis, a preallocated per-layer KV cache fed by
the strided flash-attention kernel (prefill) and a cached-decode path,
greedy/top-k sampling with vocab-parallel argmax (no logits gather).
BASELINE config 5: OPT-30B auto-sharded TP across 8x MI355X.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from ..mesh import DeviceMesh
from ..parallel.layers import tag_seed
from .decoder import CachedDecoder, DecoderBlock, KVCache  # noqa: F401


@dataclass
class OPTConfig:
    hidden_size: int = 1024
    num_layers: int = 24
    num_heads: int = 16
    vocab_size: int = 50272
    max_seq_len: int = 2048
    ffn_mult: int = 4
    layernorm_eps: float = 1e-5

    @property
    def head_dim(self):
        return self.hidden_size // self.num_heads


# reference's OPT ladder (examples/llm_serving; public OPT configs)
OPT_SPECS = {
    "125M": (768, 12, 12),
    "350M": (1024, 24, 16),
    "1.3B": (2048, 24, 32),
    "2.7B": (2560, 32, 32),
    "6.7B": (4096, 32, 32),
    "13B": (5120, 40, 40),
    "30B": (7168, 48, 56),
    "66B": (9216, 64, 72),
}


def opt_config(name: str, max_seq_len: int = 2048) -> OPTConfig:
    h, l, heads = OPT_SPECS[name]
    return OPTConfig(hidden_size=h, num_layers=l, num_heads=heads,
                     max_seq_len=max_seq_len)




class OPTBlock(DecoderBlock):
    """Sequential ln1/ln2 residuals, relu MLP."""

    def __init__(self, cfg: OPTConfig, mesh, axis, dtype, device, idx,
                 init_seed):
        super().__init__(cfg, mesh, axis, dtype, device, idx, init_seed,
                         gelu=False, parallel=False)


class OPTModel(CachedDecoder):
    """TP-sharded OPT decoder: learned positions with a +2 offset."""

    block_cls = OPTBlock

    def __init__(self, cfg: OPTConfig, mesh: Optional[DeviceMesh] = None,
                 axis: int = 1, dtype=torch.float32, device=None,
                 init_seed: int = 0):
        super().__init__(cfg, mesh, axis, dtype, device, init_seed)
        g = torch.Generator()
        g.manual_seed(tag_seed(init_seed, "wpe"))
        wpe = torch.empty(cfg.max_seq_len + 2, cfg.hidden_size,
                          dtype=torch.float32).normal_(0, 0.02, generator=g)
        self.wpe = nn.Parameter(wpe.to(dtype=dtype, device=device))

    def _embed(self, ids, pos):
        if isinstance(pos, int):
            return self.wte(ids) + self.wpe[2 + pos:2 + pos + ids.shape[1]]
        return self.wte(ids) + self.wpe[2 + pos].unsqueeze(1)

    def forward_train(self, ids: torch.Tensor) -> torch.Tensor:
        """Differentiable causal forward WITHOUT the KV cache (training/
        finetuning path — cache writes are no-grad buffers and would
        silently detach the k/v projections).  Returns full-sequence
        logits [B, S, vocab/tp]."""
        x = self._run_blocks(self._embed(ids, 0), None, 0)
        return self.lm_head(self.ln_f(x))
