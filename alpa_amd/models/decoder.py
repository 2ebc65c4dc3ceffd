"""The cached decoder that the OPT, BLOOM and CodeGen servers share.

One block (packed qkv, KV-cache write, attention, MLP), one model scaffold
(embedding, blocks, final norm, vocab-parallel head) and one set of serving
entry points: ``forward_step`` (prefill, a further chunk of tokens or one
token at a common position), ``forward_prefill`` (right-padded batch), ``forward_decode``
(one token per slot at per-slot positions, continuous batching) and the
hipGraph-captured decode loop.  A family (opt.py, bloom.py, codegen.py)
supplies its config, its embedding and what its attention needs per call
(ALiBi slopes, a rotary transform); everything that reaches
``ops.flash_attention`` / ``ops.flash_attention_varlen`` /
``ops.flash_attention_chunk`` is here.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..mesh import DeviceMesh
from ..parallel.layers import (ColumnParallelLinear, RowParallelLinear,
                               VocabParallelEmbedding)
from .generation import GenerationMixin, draw_uniforms, fused_sampling_on
from .gpt import LayerNorm


class KVCache:
    """Per-layer preallocated cache [B, heads/tp, max_len, d] (analog of
    the reference's cache-as-DistributedArrays kept on mesh,
    wrapper.py:356-371).

    fp8 (global_config.kv_cache_fp8): k and v hold float8_e4m3fn bytes and
    k_scale, v_scale [B, heads/tp, max_len] one fp32 scale per cached row
    (ops.kv_cache_append_fp8 writes them, ops.flash_attention_decode_fp8
    and ops.flash_attention_chunk_fp8 read them); otherwise k_scale and v_scale are None."""

    def __init__(self, cfg, num_layers: int, batch: int,
                 heads_per_rank: int, dtype, device,
                 max_len: Optional[int] = None, fp8: bool = False):
        d = cfg.head_dim
        max_len = max_len or cfg.max_seq_len
        self.fp8 = fp8

        def rows():
            if not fp8:
                return torch.zeros(batch, heads_per_rank, max_len, d,
                                   dtype=dtype, device=device)
            return torch.zeros(batch, heads_per_rank, max_len, d,
                               dtype=torch.uint8,
                               device=device).view(torch.float8_e4m3fn)

        self.k = [rows() for _ in range(num_layers)]
        self.v = [rows() for _ in range(num_layers)]
        self.k_scale = self.v_scale = None
        if fp8:
            self.k_scale, self.v_scale = (
                [torch.zeros(batch, heads_per_rank, max_len,
                             dtype=torch.float32, device=device)
                 for _ in range(num_layers)] for _ in range(2))
        self.length = 0

    def _lists(self):
        return [t for t in (self.k, self.v, self.k_scale, self.v_scale)
                if t is not None]

    def reorder(self, beam_idx: torch.Tensor):
        """Beam-search cache reorder (reference index-select executables,
        mesh_executable.py:1168); the scales of an fp8 cache move with
        their rows."""
        for ts in self._lists():
            for i in range(len(ts)):
                t = ts[i]
                if t.dtype == torch.float8_e4m3fn:   # gather the bytes
                    ts[i] = t.view(torch.uint8).index_select(
                        0, beam_idx).view(t.dtype)
                else:
                    ts[i] = t.index_select(0, beam_idx)

    def slots(self, s0: int, n: int) -> "KVCache":
        """A cache over slots s0 .. s0+n-1 that shares this one's memory
        (length 0), so a prefill writes straight into the shared buffers."""
        view = object.__new__(KVCache)
        view.fp8, view.length = self.fp8, 0
        view.k_scale = view.v_scale = None
        for name in ("k", "v") + (("k_scale", "v_scale") if self.fp8 else ()):
            setattr(view, name, [t[s0:s0 + n] for t in getattr(self, name)])
        return view

    def layer(self, i: int):
        """(cache_k, cache_v) of layer i as DecoderBlock takes them: the
        tensors, or (bytes, scales) pairs for an fp8 cache."""
        if self.fp8:
            return ((self.k[i], self.k_scale[i]),
                    (self.v[i], self.v_scale[i]))
        return self.k[i], self.v[i]


def _fused_write_routed(qkv, cache_k, cache_v, pos, rotary) -> bool:
    """Does this cached call take ops.qkv_cache_write?  The switch, its
    rule and the measurements behind it are on
    global_config.fused_qkv_write."""
    from ..global_env import global_config
    if global_config.fused_qkv_write in ("0", False) or \
            torch.is_grad_enabled() and qkv.requires_grad:
        return False
    return ops.qkv_cache_write_ok(qkv, cache_k, cache_v, pos, rotary)


def split_qkv_into_cache(qkv, cache_k, cache_v, pos, rotate=None,
                         rotary=None):
    """What a block does between its qkv projection and its attention call:
    qkv [B, S, h, 3, d] (the packed projection) -> (q, k, v) as [B, h, S, d],
    q and k rotated and q contiguous, with k and v written at positions
    pos_b .. pos_b + S - 1 of the cache (cache_k None: no cache).  `rotate`
    and `rotary` are the family's rotary transform in two forms: a callable
    (x, pos) -> rotated, and the (sin, cos, rotary_dim) of
    ops.qkv_cache_write.  A cached call inside that kernel's envelope
    (global_config.fused_qkv_write) is its one launch; every other call is
    the torch ops below."""
    B, S = qkv.shape[:2]
    q, k, v = (qkv[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))
    fp8 = isinstance(cache_k, tuple)
    if cache_k is not None and _fused_write_routed(qkv, cache_k, cache_v,
                                                   pos, rotary):
        # the e4m3 prefill attends over the fresh k: ask for it
        want_k = fp8 and S > 1 and pos == 0
        out = ops.qkv_cache_write(qkv, cache_k, cache_v, pos, rotary,
                                  want_k=want_k, _in_envelope=True)
        return (*out, v) if want_k else (out, k, v)
    if rotate is not None:
        q, k = rotate(q, pos), rotate(k, pos)
    q = q.contiguous()
    if fp8:
        (k8, ks), (v8, vs) = cache_k, cache_v
        ops.kv_cache_append_fp8(k, v, k8, ks, v8, vs, pos)
    elif cache_k is not None and isinstance(pos, int):
        cache_k[:, :, pos:pos + S] = k
        cache_v[:, :, pos:pos + S] = v
    elif cache_k is not None:
        assert S == 1
        bidx = torch.arange(B, device=qkv.device)
        cache_k[bidx, :, pos] = k[:, :, 0]
        cache_v[bidx, :, pos] = v[:, :, 0]
    return q, k, v


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

    def _attn(self, x, cache_k, cache_v, pos, slopes, rotate, cap,
              rotary=None):
        """pos: int — all rows sit at pos..pos+S-1 (prefill, lock-step
        decode); LongTensor [B] — one token per slot at its own position
        (continuous batching), attended with kv_lens = pos + 1.  `cap`
        fixes the attended cache capacity on that path WITHOUT the
        host-synced pos.max() — required under hipGraph capture (the
        varlen kernel masks past each slot's device-side length anyway).
        cache_k None: no cache, causal over the block's own k/v (training;
        cache writes are no-grad buffers and would detach k/v).  `rotate`
        and `rotary`: split_qkv_into_cache, which has written the cache
        when the attention calls below read it."""
        B, S, _ = x.shape
        h, d = self.heads_per_rank, self.head_dim
        q, k, v = split_qkv_into_cache(self.qkv(x).view(B, S, h, 3, d),
                                       cache_k, cache_v, pos, rotate, rotary)
        if isinstance(cache_k, tuple):
            o = self._attn_fp8(q, k, v, cache_k, cache_v, pos, slopes, cap)
        elif cache_k is None:
            o = ops.flash_attention(q, k.contiguous(), v.contiguous(),
                                    causal=True, alibi_slopes=slopes)
        elif isinstance(pos, int):
            total = pos + S
            if pos > 0 and S > 1:
                # a chunk with history: causal at the end of the cache
                o = ops.flash_attention_chunk(q, cache_k[:, :, :total],
                                              cache_v[:, :, :total],
                                              alibi_slopes=slopes)
            else:
                # a single new position sees the whole cache
                o = ops.flash_attention(q, cache_k[:, :, :total],
                                        cache_v[:, :, :total], causal=S > 1,
                                        alibi_slopes=slopes)
        else:
            total = cap or int(pos.max()) + 1
            o = ops.flash_attention_varlen(q, cache_k[:, :, :total],
                                           cache_v[:, :, :total], pos + 1,
                                           alibi_slopes=slopes)
        return self.out(o.permute(0, 2, 1, 3).reshape(B, S, h * d))

    def _attn_fp8(self, q, k, v, cache_k, cache_v, pos, slopes, cap):
        """The cached branches of _attn over an e4m3 cache that already holds
        the new rows: cache_k and cache_v are (bytes, scales).  Prefill
        attends over the fresh bf16 k/v, which is all there is to see at
        pos == 0; a chunk with history reads the cache through the e4m3
        chunk kernel; a single-token step reads it through the e4m3 decode
        kernel with kv_lens = pos + 1."""
        (k8, ks), (v8, vs) = cache_k, cache_v
        B, S = q.shape[0], q.shape[2]
        if S > 1:
            assert isinstance(pos, int)
            if pos == 0:
                return ops.flash_attention(q, k.contiguous(), v.contiguous(),
                                           causal=True, alibi_slopes=slopes)
            total = pos + S
            return ops.flash_attention_chunk_fp8(
                q, k8[:, :, :total], ks[:, :, :total], v8[:, :, :total],
                vs[:, :, :total], alibi_slopes=slopes)
        if isinstance(pos, int):
            total, lens = pos + 1, None
        else:
            total, lens = cap or int(pos.max()) + 1, pos + 1
        return ops.flash_attention_decode_fp8(
            q, k8[:, :, :total], ks[:, :, :total], v8[:, :, :total],
            vs[:, :, :total], kv_lens=lens, alibi_slopes=slopes)

    def _mlp(self, y):
        y = self.fc1(y)
        return self.fc2(y if self.gelu else torch.nn.functional.relu(y))

    def forward(self, x, cache_k, cache_v, pos, slopes=None, rotate=None,
                cap=None, rotary=None):
        if self.parallel:
            y = self.ln(x)
            return x + self._attn(y, cache_k, cache_v, pos, slopes, rotate,
                                  cap, rotary) + self._mlp(y)
        x = x + self._attn(self.ln1(x), cache_k, cache_v, pos, slopes,
                           rotate, cap, rotary)
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
        """Per-call keyword arguments of the blocks (slopes, rotate,
        rotary)."""
        return {}

    def _run_blocks(self, x, cache, pos, cap=None):
        kw = self._attn_args()
        for i, blk in enumerate(self.blocks):
            ck, cv = cache.layer(i) if cache is not None else (None, None)
            x = blk(x, ck, cv, pos, cap=cap, **kw)
        return x

    def new_cache(self, batch: int, max_len: Optional[int] = None
                  ) -> KVCache:
        from ..global_env import global_config
        return KVCache(self.cfg, self.cfg.num_layers, batch,
                       self.heads_per_rank, self.dtype, self.device_,
                       max_len=max_len, fp8=global_config.kv_cache_fp8)

    def forward_step(self, ids: torch.Tensor, cache: KVCache
                     ) -> torch.Tensor:
        """ids [B, S]: the S tokens at positions cache.length ..
        cache.length + S - 1 of every slot: a whole prompt, a further chunk
        of one (chunked prefill, draft verification, a multi-token turn;
        ops.flash_attention_chunk) or one token.  Returns last-position
        logits [B, vocab/tp]."""
        S = ids.shape[1]
        pos = cache.length
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
                        max_new_tokens: int, do_sample: bool = False,
                        temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0,
                        generator: Optional[torch.Generator] = None
                        ) -> "_GraphedDecode":
        """Prefill + capture now; `.run()` replays the decode loop
        (single use — the cache advances).  Lets benchmarks time the
        replay loop separately from the one-time capture."""
        return _GraphedDecode(self, prompt_ids, max_new_tokens, do_sample,
                              temperature, top_k, top_p, generator)

    @torch.no_grad()
    def generate_graphed(self, prompt_ids: torch.Tensor,
                         max_new_tokens: int, do_sample: bool = False,
                         temperature: float = 1.0, top_k: int = 0,
                         top_p: float = 1.0,
                         generator: Optional[torch.Generator] = None
                         ) -> torch.Tensor:
        """Greedy (default) or sampled generate with the DECODE STEP
        hipGraph-captured.  With do_sample the step ends in
        ops.sample_logits (global_config.fused_sampling must be on): the
        uniforms of all steps are drawn before capture and the captured
        step takes its row by a device step counter, so the result equals
        generate(do_sample=True) with an equally seeded generator.

        Eager decode is host-bound (~23 us/op measured: OPT-66B 28.1
        ms/token = ~1200 op dispatches) — capturing one whole decode
        step (including the greedy-token feedback and the device-side
        length increment) reduces the per-token host work to one graph
        replay + one token copy-out.  Everything dynamic lives in
        device tensors updated in place: the varlen attention masks by
        lens, the cache scatter and wpe gather index by lens, and the
        cache view is a fixed capacity (prompt + max_new_tokens).
        Single-mesh (tp=1) path; requires CUDA."""
        return self.graphed_decoder(prompt_ids, max_new_tokens, do_sample,
                                    temperature, top_k, top_p,
                                    generator).run()


class _GraphedDecode:
    """See CachedDecoder.generate_graphed."""

    @torch.no_grad()
    def __init__(self, model, prompt_ids, max_new_tokens, do_sample=False,
                 temperature=1.0, top_k=0, top_p=1.0, generator=None):
        assert prompt_ids.is_cuda and (
            model.mesh is None or model.mesh.axis_size(model.axis) == 1)
        B, S0 = prompt_ids.shape
        dev = prompt_ids.device
        self.model, self.prompt_ids = model, prompt_ids
        self.max_new = max_new_tokens
        cap = S0 + max_new_tokens
        cache = model.new_cache(B, max_len=cap)
        logits = model.forward_step(prompt_ids, cache)
        if do_sample:
            # the multinomial draw of the torch path reads the generator on
            # the host: only the kernel's draw can be captured
            assert fused_sampling_on(), \
                "a sampled graph needs global_config.fused_sampling"
            us = draw_uniforms(max_new_tokens, B, generator, dev)
            # row of `us` the next step consumes, advanced inside the graph
            nstep = torch.ones(1, dtype=torch.long, device=dev)

            def pick(lg, u):
                return model.sample_token(lg, temperature, top_k, top_p,
                                          u=u)

            tok = pick(logits, us[0])
        else:
            tok = model.greedy_token(logits)
        tok = self.tok = tok.reshape(B, 1).clone()
        lens = self.lens = torch.full((B,), S0, dtype=torch.long,
                                      device=dev)
        out = self.out = torch.empty(B, max_new_tokens,
                                     dtype=prompt_ids.dtype, device=dev)
        out[:, 0] = tok[:, 0]

        def step():
            lg = model.forward_decode(tok, cache, lens, cap=cap)
            if do_sample:
                nxt = pick(lg, us.index_select(0, nstep)[0])
                nstep.add_(1)
            else:
                nxt = model.greedy_token(lg)
            lens.add_(1)
            tok.copy_(nxt.reshape(B, 1))

        # warmup on a side stream (standard capture recipe), then capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        # roll back the warmup step's state mutations
        lens.fill_(S0)
        tok[:, 0] = out[:, 0]
        if do_sample:
            nstep.fill_(1)
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
