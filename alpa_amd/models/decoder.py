"""The cached decoder that the OPT, BLOOM and CodeGen servers share.

One block (packed qkv, KV-cache write, attention, MLP), one model scaffold
(embedding, blocks, final norm, vocab-parallel head) and one set of serving
entry points: ``forward_step`` (prefill / single-token decode at a common
position), ``forward_prefill`` (right-padded batch), ``forward_decode``
(one token per slot at per-slot positions, continuous batching) and the
hipGraph-captured decode loop.  A family (opt.py, bloom.py, codegen.py)
supplies its config, its embedding and what its attention needs per call
(ALiBi slopes, a rotary transform); everything that reaches
``ops.flash_attention`` / ``ops.flash_attention_varlen`` is here.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..mesh import DeviceMesh
from ..parallel.layers import (ColumnParallelLinear, RowParallelLinear,
                               VocabParallelEmbedding)
from .generation import GenerationMixin
from .gpt import LayerNorm


class KVCache:
    """Per-layer preallocated cache [B, heads/tp, max_len, d] (analog of
    the reference's cache-as-DistributedArrays kept on mesh,
    wrapper.py:356-371)."""

    def __init__(self, cfg, num_layers: int, batch: int,
                 heads_per_rank: int, dtype, device,
                 max_len: Optional[int] = None):
        d = cfg.head_dim
        max_len = max_len or cfg.max_seq_len
        self.k = [torch.zeros(batch, heads_per_rank, max_len, d,
                              dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.v = [torch.zeros(batch, heads_per_rank, max_len, d,
                              dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.length = 0

    def reorder(self, beam_idx: torch.Tensor):
        """Beam-search cache reorder (reference index-select executables,
        mesh_executable.py:1168)."""
        for i in range(len(self.k)):
            self.k[i] = self.k[i].index_select(0, beam_idx)
            self.v[i] = self.v[i].index_select(0, beam_idx)


class DecoderBlock(nn.Module):
    """Attention + MLP block.  `gelu`: fc1 fuses bias+GeLU (BLOOM, CodeGen)
    instead of a relu after a plain fc1 (OPT).  `parallel`: one LayerNorm
    `ln` feeds attention and MLP side by side (CodeGen, GPT-J) instead of
    the sequential `ln1` / `ln2` residuals (OPT, BLOOM)."""

    def __init__(self, cfg, mesh, axis, dtype, device, idx, init_seed,
                 gelu: bool, parallel: bool):
        super().__init__()
        tp = mesh.axis_size(axis) if mesh is not None else 1
        self.heads_per_rank = cfg.num_heads // tp
        self.head_dim = cfg.head_dim
        self.gelu, self.parallel = gelu, parallel
        hidden, ffn = cfg.hidden_size, cfg.ffn_mult * cfg.hidden_size

        def linear(cls, n_in, n_out, tag, **kw):
            return cls(n_in, n_out, mesh, axis, dtype=dtype, device=device,
                       init_seed=init_seed, init_tag=f"b{idx}.{tag}", **kw)

        def norm():
            return LayerNorm(hidden, cfg.layernorm_eps, dtype, device)

        if parallel:
            self.ln = norm()
        else:
            self.ln1, self.ln2 = norm(), norm()
        self.qkv = linear(ColumnParallelLinear, hidden, 3 * hidden, "qkv")
        self.out = linear(RowParallelLinear, hidden, hidden, "out")
        self.fc1 = linear(ColumnParallelLinear, hidden, ffn, "fc1",
                          gelu=gelu)
        self.fc2 = linear(RowParallelLinear, ffn, hidden, "fc2")

    def _attn(self, x, cache_k, cache_v, pos, slopes, rotate, cap):
        """pos: int — all rows sit at pos..pos+S-1 (prefill, lock-step
        decode); LongTensor [B] — one token per slot at its own position
        (continuous batching), attended with kv_lens = pos + 1.  `cap`
        fixes the attended cache capacity on that path WITHOUT the
        host-synced pos.max() — required under hipGraph capture (the
        varlen kernel masks past each slot's device-side length anyway).
        cache_k None: no cache, causal over the block's own k/v (training;
        cache writes are no-grad buffers and would detach k/v)."""
        B, S, _ = x.shape
        h, d = self.heads_per_rank, self.head_dim
        qkv = self.qkv(x).view(B, S, h, 3, d)
        q, k, v = (qkv[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))
        if rotate is not None:
            q, k = rotate(q, pos), rotate(k, pos)
        q = q.contiguous()
        if cache_k is None:
            o = ops.flash_attention(q, k.contiguous(), v.contiguous(),
                                    causal=True, alibi_slopes=slopes)
        elif isinstance(pos, int):
            total = pos + S
            cache_k[:, :, pos:total] = k
            cache_v[:, :, pos:total] = v
            # a single new position sees the whole cache; a chunk with
            # history would need a causal offset (forward_step refuses it)
            o = ops.flash_attention(q, cache_k[:, :, :total],
                                    cache_v[:, :, :total], causal=S > 1,
                                    alibi_slopes=slopes)
        else:
            assert S == 1
            bidx = torch.arange(B, device=x.device)
            cache_k[bidx, :, pos] = k[:, :, 0]
            cache_v[bidx, :, pos] = v[:, :, 0]
            total = cap or int(pos.max()) + 1
            o = ops.flash_attention_varlen(q, cache_k[:, :, :total],
                                           cache_v[:, :, :total], pos + 1,
                                           alibi_slopes=slopes)
        return self.out(o.permute(0, 2, 1, 3).reshape(B, S, h * d))

    def _mlp(self, y):
        y = self.fc1(y)
        return self.fc2(y if self.gelu else torch.nn.functional.relu(y))

    def forward(self, x, cache_k, cache_v, pos, slopes=None, rotate=None,
                cap=None):
        if self.parallel:
            y = self.ln(x)
            return x + self._attn(y, cache_k, cache_v, pos, slopes, rotate,
                                  cap) + self._mlp(y)
        x = x + self._attn(self.ln1(x), cache_k, cache_v, pos, slopes,
                           rotate, cap)
        return x + self._mlp(self.ln2(x))


class CachedDecoder(nn.Module, GenerationMixin):
    """TP-sharded decoder with KV-cache generation (greedy/sampling/beam
    from GenerationMixin).  A family names its block class (a DecoderBlock
    with the activation and residual layout fixed) and implements `_embed`;
    `_attn_args` is what its blocks need per call."""

    block_cls = None
    max_head_dim = 256

    def __init__(self, cfg, mesh: Optional[DeviceMesh] = None,
                 axis: int = 1, dtype=torch.float32, device=None,
                 init_seed: int = 0):
        super().__init__()
        self.cfg = cfg
        assert cfg.head_dim <= self.max_head_dim, (
            f"head_dim {cfg.head_dim} > {self.max_head_dim} unsupported: "
            "the attention kernels take head_dim up to 256 (dims in (128, "
            "256] use the blocked hipBLASLt attention path) and ALiBi "
            "slopes only up to 128")
        self.mesh, self.axis = mesh, axis
        tp = mesh.axis_size(axis) if mesh is not None else 1
        self.heads_per_rank = cfg.num_heads // tp
        self.wte = VocabParallelEmbedding(cfg.vocab_size, cfg.hidden_size,
                                          mesh, axis, dtype=dtype,
                                          device=device, init_seed=init_seed,
                                          init_tag="wte")
        self.blocks = nn.ModuleList([
            self.block_cls(cfg, mesh, axis, dtype, device, i, init_seed)
            for i in range(cfg.num_layers)
        ])
        self.ln_f = LayerNorm(cfg.hidden_size, cfg.layernorm_eps, dtype,
                              device)
        self.lm_head = ColumnParallelLinear(cfg.hidden_size, cfg.vocab_size,
                                            mesh, axis, bias=False,
                                            dtype=dtype, device=device,
                                            init_seed=init_seed,
                                            init_tag="lm_head")
        self.lm_head._fp8_exclude = True  # logits GEMM stays bf16
        self.dtype = dtype
        self.device_ = device

    def _embed(self, ids: torch.Tensor, pos) -> torch.Tensor:
        """ids [B, S] -> [B, S, hidden]; pos as in DecoderBlock._attn."""
        raise NotImplementedError

    def _attn_args(self) -> dict:
        """Per-call keyword arguments of the blocks (slopes, rotate)."""
        return {}

    def _run_blocks(self, x, cache, pos, cap=None):
        kw = self._attn_args()
        for i, blk in enumerate(self.blocks):
            ck, cv = (cache.k[i], cache.v[i]) if cache is not None \
                else (None, None)
            x = blk(x, ck, cv, pos, cap=cap, **kw)
        return x

    def new_cache(self, batch: int, max_len: Optional[int] = None
                  ) -> KVCache:
        return KVCache(self.cfg, self.cfg.num_layers, batch,
                       self.heads_per_rank, self.dtype, self.device_,
                       max_len=max_len)

    def forward_step(self, ids: torch.Tensor, cache: KVCache
                     ) -> torch.Tensor:
        """ids [B, S] (prefill) or [B, 1] (decode). Returns last-position
        logits [B, vocab/tp]."""
        S = ids.shape[1]
        pos = cache.length
        # chunked decode with history would need a causal-offset mask in the
        # kernel; prefill (pos==0) and single-token decode cover serving
        assert pos == 0 or S == 1, "chunked decode with history unsupported"
        x = self._run_blocks(self._embed(ids, pos), cache, pos)
        cache.length += S
        return self.lm_head(self.ln_f(x[:, -1:]))[:, 0]

    @torch.no_grad()
    def forward_prefill(self, ids: torch.Tensor, lens: torch.Tensor,
                        cache: KVCache) -> torch.Tensor:
        """Batched variable-length prefill: ids [n, Smax] right-padded
        prompts, lens [n] true lengths.  ONE causal pass prefills every
        slot (padding rows only contaminate padding rows under the
        causal mask; ALiBi biases depend only on relative positions, so
        this holds for BLOOM too); returns each slot's last-real-position
        logits [n, vocab/tp].  The continuous batcher admits all pending
        requests through this instead of per-slot prefills (reference 1-D
        batching, opt_model_1d.py)."""
        B, S = ids.shape
        x = self._run_blocks(self._embed(ids, 0), cache, 0)
        cache.length = S
        idx = (lens.to(ids.device) - 1).clamp(min=0)
        x_last = x[torch.arange(B, device=ids.device), idx].unsqueeze(1)
        return self.lm_head(self.ln_f(x_last))[:, 0]

    @torch.no_grad()
    def forward_decode(self, tok: torch.Tensor, cache: KVCache,
                       lens: torch.Tensor, cap=None) -> torch.Tensor:
        """Varlen decode (continuous batching): tok [B, 1] next token per
        slot, lens [B] tokens already cached per slot.  Returns logits
        [B, vocab/tp].  The caller owns per-slot length bookkeeping
        (cache.length is unused on this path)."""
        x = self._run_blocks(self._embed(tok, lens), cache, lens, cap)
        return self.lm_head(self.ln_f(x))[:, 0]

    @torch.no_grad()
    def graphed_decoder(self, prompt_ids: torch.Tensor,
                        max_new_tokens: int) -> "_GraphedDecode":
        """Prefill + capture now; `.run()` replays the decode loop
        (single use — the cache advances).  Lets benchmarks time the
        replay loop separately from the one-time capture."""
        return _GraphedDecode(self, prompt_ids, max_new_tokens)

    @torch.no_grad()
    def generate_graphed(self, prompt_ids: torch.Tensor,
                         max_new_tokens: int) -> torch.Tensor:
        """Greedy generate with the DECODE STEP hipGraph-captured.

        Eager decode is host-bound (~23 us/op measured: OPT-66B 28.1
        ms/token = ~1200 op dispatches) — capturing one whole decode
        step (including the greedy-token feedback and the device-side
        length increment) reduces the per-token host work to one graph
        replay + one token copy-out.  Everything dynamic lives in
        device tensors updated in place: the varlen attention masks by
        lens, the cache scatter and wpe gather index by lens, and the
        cache view is a fixed capacity (prompt + max_new_tokens).
        Single-mesh (tp=1) path; requires CUDA."""
        return self.graphed_decoder(prompt_ids, max_new_tokens).run()


class _GraphedDecode:
    """See CachedDecoder.generate_graphed."""

    @torch.no_grad()
    def __init__(self, model, prompt_ids, max_new_tokens):
        assert prompt_ids.is_cuda and (
            model.mesh is None or model.mesh.axis_size(model.axis) == 1)
        B, S0 = prompt_ids.shape
        self.model, self.prompt_ids = model, prompt_ids
        self.max_new = max_new_tokens
        cap = S0 + max_new_tokens
        cache = model.new_cache(B, max_len=cap)
        logits = model.forward_step(prompt_ids, cache)
        tok = self.tok = model.greedy_token(logits).reshape(B, 1).clone()
        lens = self.lens = torch.full((B,), S0, dtype=torch.long,
                                      device=prompt_ids.device)
        out = self.out = torch.empty(B, max_new_tokens,
                                     dtype=prompt_ids.dtype,
                                     device=prompt_ids.device)
        out[:, 0] = tok[:, 0]

        def step():
            lg = model.forward_decode(tok, cache, lens, cap=cap)
            nxt = model.greedy_token(lg).reshape(B, 1)
            lens.add_(1)
            tok.copy_(nxt)

        # warmup on a side stream (standard capture recipe), then capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        # roll back the warmup step's state mutations
        lens.fill_(S0)
        tok[:, 0] = out[:, 0]
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            step()

    @torch.no_grad()
    def run(self) -> torch.Tensor:
        # capture ran no work; replay i generates token i+1
        for i in range(1, self.max_new):
            self.graph.replay()
            self.out[:, i] = self.tok[:, 0]
        return torch.cat([self.prompt_ids, self.out], dim=1)
