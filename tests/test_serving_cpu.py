"""Serving tests: OPT generation with KV cache (serial vs TP2 parity,
cache-vs-recompute consistency), HTTP controller (reference:
alpa/serve + examples/llm_serving)."""
import pytest
import torch

from dist_utils import run_distributed

import alpa_amd as aa
from alpa_amd.models.opt import KVCache, OPTConfig, OPTModel
from alpa_amd.serve import Controller

CFG = OPTConfig(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
                max_seq_len=64)


def build_opt(mesh=None, axis=1):
    return OPTModel(CFG, mesh, axis, torch.float32, None, init_seed=13)


def test_cache_decode_matches_full_recompute():
    """Decoding with the KV cache must equal re-running the whole prefix."""
    torch.manual_seed(0)
    m = build_opt()
    ids = torch.randint(0, CFG.vocab_size, (2, 8))
    # incremental: prefill 8 then decode 3
    cache = m.new_cache(2)
    logits = m.forward_step(ids, cache)
    seq = ids
    for _ in range(3):
        nxt = m.greedy_token(logits).unsqueeze(1)
        seq = torch.cat([seq, nxt], dim=1)
        logits = m.forward_step(nxt, cache)
    # full recompute of the final prefix
    cache2 = m.new_cache(2)
    logits_full = m.forward_step(seq, cache2)
    torch.testing.assert_close(logits, logits_full, rtol=2e-4, atol=2e-4)


def test_generate_shapes_and_determinism():
    m = build_opt()
    ids = torch.randint(0, CFG.vocab_size, (2, 5))
    out1 = m.generate(ids, max_new_tokens=6)
    out2 = m.generate(ids, max_new_tokens=6)
    assert out1.shape == (2, 11)
    torch.testing.assert_close(out1, out2)
    assert torch.equal(out1[:, :5], ids)


def _tp_gen_worker(rank, world_size):
    mesh = aa.full_mesh((1, world_size))
    m = build_opt(mesh, 1)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, CFG.vocab_size, (2, 5), generator=g)
    return m.generate(ids, max_new_tokens=6)


def test_tp2_generation_matches_serial():
    """Auto-sharded TP serving must emit exactly the serial tokens."""
    m = build_opt()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, CFG.vocab_size, (2, 5), generator=g)
    serial = m.generate(ids, max_new_tokens=6)
    results = run_distributed(_tp_gen_worker, world_size=2, timeout=300)
    for r in results:
        torch.testing.assert_close(r, serial)


def test_kv_cache_reorder():
    cache = KVCache(CFG, 2, batch=4, heads_per_rank=4,
                    dtype=torch.float32, device=None)
    cache.k[0][:, 0, 0, 0] = torch.tensor([0., 1., 2., 3.])
    cache.reorder(torch.tensor([3, 2, 1, 0]))
    assert cache.k[0][:, 0, 0, 0].tolist() == [3., 2., 1., 0.]


def test_http_controller():
    from starlette.testclient import TestClient
    m = build_opt()
    c = Controller()
    c.register_model("opt-test",
                     lambda ids, mt: m.generate(ids, max_new_tokens=mt))
    client = TestClient(c.asgi_app())
    r = client.get("/models")
    assert r.json() == {"models": ["opt-test"]}
    r = client.post("/completions", json={
        "model": "opt-test", "prompt_ids": [[1, 2, 3]], "max_tokens": 4})
    out = r.json()["output_ids"]
    assert len(out) == 1 and len(out[0]) == 7
    assert out[0][:3] == [1, 2, 3]
    r = client.post("/completions", json={"model": "opt-test"})
    assert r.status_code == 400


# ---------------------------------------------------------------------------
# Beam search (reference: llm_serving wrapper beam path with index-select
# cache reorder, model/wrapper.py:115-182)
# ---------------------------------------------------------------------------


def test_log_probs_topk_matches_log_softmax():
    torch.manual_seed(3)
    m = build_opt()
    logits = torch.randn(4, CFG.vocab_size)
    lp, idx = m._log_probs_topk(logits, 5)
    ref = torch.log_softmax(logits.float(), dim=-1)
    ref_v, ref_i = ref.topk(5, dim=-1)
    torch.testing.assert_close(lp, ref_v, rtol=1e-5, atol=1e-5)
    assert torch.equal(idx, ref_i)


def test_beam1_equals_greedy():
    torch.manual_seed(4)
    m = build_opt()
    ids = torch.randint(0, CFG.vocab_size, (2, 6))
    greedy = m.generate(ids, 8)
    beam = m.beam_search(ids, 8, num_beams=1)
    assert torch.equal(greedy, beam)


def test_beam_search_shapes_and_eos():
    torch.manual_seed(5)
    m = build_opt()
    ids = torch.randint(0, CFG.vocab_size, (2, 4))
    out = m.beam_search(ids, 10, num_beams=4)
    assert out.shape == (2, 14)
    # with eos: once a sequence ends, its tail is all eos
    eos = 7
    out = m.beam_search(ids, 10, num_beams=4, eos_token=eos)
    for row in out:
        tail = row[4:]
        hits = (tail == eos).nonzero()
        if len(hits):
            first = int(hits[0])
            assert bool((tail[first:] == eos).all())


def _tp_beam_worker(rank, world_size):
    mesh = aa.mesh.full_mesh((1, world_size))
    m = build_opt(mesh, axis=1)
    torch.manual_seed(6)
    ids = torch.randint(0, CFG.vocab_size, (2, 5))
    return m.beam_search(ids, 6, num_beams=3, eos_token=2)


def test_tp2_beam_matches_serial():
    """Vocab-parallel global top-k + local cache reorder reproduce the
    serial beam search exactly."""
    torch.manual_seed(6)
    serial = build_opt().beam_search(
        torch.randint(0, CFG.vocab_size, (2, 5)), 6, num_beams=3,
        eos_token=2)
    results = run_distributed(_tp_beam_worker, world_size=2, timeout=300)
    for r in results:
        assert torch.equal(torch.as_tensor(r), serial), (r, serial)


# ---------------------------------------------------------------------------
# CodeGen (rotary, GPT-J parallel-residual; reference codegen_model.py)
# ---------------------------------------------------------------------------


def test_codegen_cache_decode_matches_recompute():
    """Rotary positions must line up between prefill and cached decode."""
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    torch.manual_seed(8)
    cfg = CodeGenConfig(hidden_size=64, num_layers=2, num_heads=4,
                        vocab_size=96, max_seq_len=64, rotary_dim=8)
    m = CodeGenModel(cfg, init_seed=17)
    ids = torch.randint(0, 96, (2, 8))
    cache = m.new_cache(2)
    logits = m.forward_step(ids, cache)
    seq = ids
    for _ in range(3):
        nxt = m.greedy_token(logits).unsqueeze(1)
        seq = torch.cat([seq, nxt], dim=1)
        logits = m.forward_step(nxt, cache)
    logits_full = m.forward_step(seq, m.new_cache(2))
    torch.testing.assert_close(logits, logits_full, rtol=2e-4, atol=2e-4)


def test_codegen_generate_and_beam():
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    torch.manual_seed(9)
    cfg = CodeGenConfig(hidden_size=64, num_layers=2, num_heads=4,
                        vocab_size=96, max_seq_len=64, rotary_dim=8)
    m = CodeGenModel(cfg, init_seed=17)
    ids = torch.randint(0, 96, (2, 6))
    out = m.generate(ids, max_new_tokens=5)
    assert out.shape == (2, 11)
    beam1 = m.beam_search(ids, 5, num_beams=1)
    assert torch.equal(out, beam1)


def test_rotary_apply_norm_preserving():
    """Rotation preserves pair norms and leaves dims >= rotary_dim
    untouched."""
    from alpa_amd.models.codegen import apply_rotary, rotary_tables
    torch.manual_seed(10)
    sin, cos = rotary_tables(8, 32, torch.float32, None)
    x = torch.randn(1, 2, 5, 16)
    y = apply_rotary(x, sin, cos, 3, 8)
    torch.testing.assert_close(y[..., 8:], x[..., 8:])
    xn = x[..., :8].view(1, 2, 5, 4, 2).norm(dim=-1)
    yn = y[..., :8].view(1, 2, 5, 4, 2).norm(dim=-1)
    torch.testing.assert_close(xn, yn, rtol=1e-5, atol=1e-5)


def _tp_codegen_worker(rank, world_size):
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    mesh = aa.mesh.full_mesh((1, world_size))
    cfg = CodeGenConfig(hidden_size=64, num_layers=2, num_heads=4,
                        vocab_size=96, max_seq_len=64, rotary_dim=8)
    m = CodeGenModel(cfg, mesh, 1, init_seed=17)
    torch.manual_seed(11)
    ids = torch.randint(0, 96, (2, 6))
    return m.generate(ids, max_new_tokens=4)


def test_tp2_codegen_matches_serial():
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    cfg = CodeGenConfig(hidden_size=64, num_layers=2, num_heads=4,
                        vocab_size=96, max_seq_len=64, rotary_dim=8)
    m = CodeGenModel(cfg, init_seed=17)
    torch.manual_seed(11)
    ids = torch.randint(0, 96, (2, 6))
    serial = m.generate(ids, max_new_tokens=4)
    results = run_distributed(_tp_codegen_worker, world_size=2, timeout=300)
    for r in results:
        assert torch.equal(torch.as_tensor(r), serial)


# ---------------------------------------------------------------------------
# BLOOM (ALiBi; reference bloom_model.py)
# ---------------------------------------------------------------------------


def test_alibi_slopes_ladder():
    from alpa_amd.models.bloom import alibi_slopes
    s8 = alibi_slopes(8)
    torch.testing.assert_close(s8, torch.tensor(
        [2.0 ** -(i + 1) for i in range(8)]))
    s12 = alibi_slopes(12)
    assert s12.shape == (12,) and bool((s12 > 0).all())


def test_alibi_reference_math():
    """ops.reference with alibi == manual softmax with the bias matrix
    (incl. the cached-decode q-position offset)."""
    from alpa_amd.ops import reference as ref
    torch.manual_seed(12)
    B, H, S, Skv, D = 1, 2, 3, 8, 16
    q = torch.randn(B, H, S, D)
    k = torch.randn(B, H, Skv, D)
    v = torch.randn(B, H, Skv, D)
    slopes = torch.tensor([0.5, 0.25])
    o, lse = ref.attention_fwd(q, k, v, causal=False, softmax_scale=0.3,
                               alibi=slopes)
    qpos = torch.arange(S) + (Skv - S)
    bias = slopes.view(1, H, 1, 1) * (
        torch.arange(Skv).view(1, 1, 1, Skv) -
        qpos.view(1, 1, S, 1)).float()
    s = q @ k.transpose(-1, -2) * 0.3 + bias
    torch.testing.assert_close(o, torch.softmax(s, -1) @ v, rtol=1e-5,
                               atol=1e-5)


def test_bloom_cache_decode_matches_recompute():
    """ALiBi bias must track ABSOLUTE positions through the KV cache."""
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    torch.manual_seed(13)
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=64)
    m = BloomModel(cfg, init_seed=19)
    ids = torch.randint(0, 96, (2, 8))
    cache = m.new_cache(2)
    logits = m.forward_step(ids, cache)
    seq = ids
    for _ in range(3):
        nxt = m.greedy_token(logits).unsqueeze(1)
        seq = torch.cat([seq, nxt], dim=1)
        logits = m.forward_step(nxt, cache)
    logits_full = m.forward_step(seq, m.new_cache(2))
    torch.testing.assert_close(logits, logits_full, rtol=2e-4, atol=2e-4)


def _tp_bloom_worker(rank, world_size):
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    mesh = aa.mesh.full_mesh((1, world_size))
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=64)
    m = BloomModel(cfg, mesh, 1, init_seed=19)
    torch.manual_seed(14)
    ids = torch.randint(0, 96, (2, 6))
    return m.generate(ids, max_new_tokens=4)


def test_tp2_bloom_matches_serial():
    """TP shards get DIFFERENT slope subsets — generation must still equal
    serial exactly."""
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=64)
    m = BloomModel(cfg, init_seed=19)
    torch.manual_seed(14)
    ids = torch.randint(0, 96, (2, 6))
    serial = m.generate(ids, max_new_tokens=4)
    results = run_distributed(_tp_bloom_worker, world_size=2, timeout=300)
    for r in results:
        assert torch.equal(torch.as_tensor(r), serial)


def test_sampling_top_k_top_p():
    """sample_token respects top-k/top-p supports and temperature; greedy
    is the temperature->0 limit."""
    torch.manual_seed(15)
    m = build_opt()
    logits = torch.randn(4, CFG.vocab_size) * 3
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        t = m.sample_token(logits, top_k=5, generator=g)
        ref_top5 = logits.topk(5, -1).indices
        for b in range(4):
            assert t[b] in ref_top5[b]
    # top_p=tiny keeps only the argmax
    t = m.sample_token(logits, top_p=1e-9, generator=g)
    assert torch.equal(t, logits.argmax(-1))
    # near-zero temperature concentrates on the argmax
    t = m.sample_token(logits, temperature=1e-5, generator=g)
    assert torch.equal(t, logits.argmax(-1))


def _tp_sample_worker(rank, world_size):
    mesh = aa.mesh.full_mesh((1, world_size))
    m = build_opt(mesh, axis=1)
    torch.manual_seed(16)
    ids = torch.randint(0, CFG.vocab_size, (2, 5))
    g = torch.Generator().manual_seed(99)
    return m.generate(ids, 5, do_sample=True, top_k=10, generator=g)


def test_tp2_sampling_matches_serial():
    """Sampled decode under TP: identical candidate sets + shared RNG keep
    every rank (and the serial oracle) in lockstep."""
    m = build_opt()
    torch.manual_seed(16)
    ids = torch.randint(0, CFG.vocab_size, (2, 5))
    g = torch.Generator().manual_seed(99)
    serial = m.generate(ids, 5, do_sample=True, top_k=10, generator=g)
    results = run_distributed(_tp_sample_worker, world_size=2, timeout=300)
    for r in results:
        assert torch.equal(torch.as_tensor(r), serial)


# ---------------------------------------------------------------------------
# Continuous batching (reference opt_model_1d / wrapper_1d)
# ---------------------------------------------------------------------------


def test_varlen_attention_reference():
    """Per-batch kv_lens masking == per-request separate attention."""
    from alpa_amd import ops
    torch.manual_seed(20)
    B, H, D = 3, 2, 16
    q = torch.randn(B, H, 1, D)
    k = torch.randn(B, H, 8, D)
    v = torch.randn(B, H, 8, D)
    lens = torch.tensor([3, 8, 5])
    o = ops.flash_attention_varlen(q, k, v, lens)
    for b, L in enumerate(lens.tolist()):
        ob = ops.flash_attention(q[b:b + 1], k[b:b + 1, :, :L],
                                 v[b:b + 1, :, :L], causal=False)
        torch.testing.assert_close(o[b:b + 1], ob, rtol=1e-5, atol=1e-5)


def _check_batcher_matches_solo(m, max_batch):
    from alpa_amd.serve.batching import ContinuousBatcher, GenRequest
    prompts = [torch.randint(0, m.cfg.vocab_size, (n,))
               for n in (5, 9, 3, 7)]
    want = [m.generate(p.view(1, -1), max_new_tokens=6)[0, len(p):]
            for p in prompts]
    cb = ContinuousBatcher(m, max_batch=max_batch)
    reqs = [GenRequest(p, max_new_tokens=6) for p in prompts]
    for r in reqs:
        cb.submit(r)
    cb.run_all()
    for r, w in zip(reqs, want):
        assert r.done
        assert r.output == w.tolist(), (r.output, w.tolist())


def test_continuous_batching_matches_per_request():
    """Staggered requests through the slot batcher produce exactly the
    tokens each request would get alone (greedy)."""
    torch.manual_seed(21)
    _check_batcher_matches_solo(build_opt(), max_batch=2)


@pytest.mark.parametrize("max_batch", [2, 3])
@pytest.mark.parametrize("seed", [21, 31])
def test_continuous_batching_matches_per_request_bloom(seed, max_batch):
    """The same through BLOOM: per-slot decode with ALiBi slopes (the
    bias of slot b is taken from its own length, not the batch's)."""
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    torch.manual_seed(seed)
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=64)
    _check_batcher_matches_solo(BloomModel(cfg, init_seed=19), max_batch)


def test_codegen_forward_decode_not_implemented():
    """Rotary takes one int position for the whole batch: per-slot decode
    must refuse, by name, not rotate every slot to a wrong position."""
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    cfg = CodeGenConfig(hidden_size=64, num_layers=2, num_heads=4,
                        vocab_size=96, max_seq_len=64, rotary_dim=8)
    m = CodeGenModel(cfg, init_seed=17)
    cache = m.new_cache(2, max_len=16)
    assert cache.k[0].shape[2] == 16
    with pytest.raises(NotImplementedError, match="per-slot positions"):
        m.forward_decode(torch.zeros(2, 1, dtype=torch.long), cache,
                         torch.tensor([3, 5]))


def test_continuous_batching_eos_frees_slot():
    from alpa_amd.serve.batching import ContinuousBatcher, GenRequest
    torch.manual_seed(22)
    m = build_opt()
    p = torch.randint(0, CFG.vocab_size, (4,))
    solo = m.generate(p.view(1, -1), max_new_tokens=8)[0, 4:].tolist()
    eos = solo[2]
    cb = ContinuousBatcher(m, max_batch=1)
    r = GenRequest(p, max_new_tokens=8, eos_token=eos)
    cb.submit(r)
    cb.run_all()
    # stops at the FIRST occurrence of eos in the greedy stream
    expect = solo[:solo.index(eos) + 1]
    assert r.done and r.output == expect
    assert cb.num_active == 0


def _tp_batcher_worker(rank, world_size):
    from alpa_amd.serve.batching import ContinuousBatcher, GenRequest
    mesh = aa.mesh.full_mesh((1, world_size))
    m = build_opt(mesh, axis=1)
    torch.manual_seed(23)
    prompts = [torch.randint(0, CFG.vocab_size, (n,)) for n in (4, 7)]
    cb = ContinuousBatcher(m, max_batch=2)
    reqs = [GenRequest(p, max_new_tokens=4) for p in prompts]
    for r in reqs:
        cb.submit(r)
    cb.run_all()
    return [r.output for r in reqs]


def test_tp2_continuous_batching_matches_serial():
    """The slot batcher under TP: vocab-parallel greedy + varlen decode
    stay in SPMD lockstep and match solo serial decodes."""
    m = build_opt()
    torch.manual_seed(23)
    prompts = [torch.randint(0, CFG.vocab_size, (n,)) for n in (4, 7)]
    want = [m.generate(p.view(1, -1), max_new_tokens=4)[0, len(p):].tolist()
            for p in prompts]
    results = run_distributed(_tp_batcher_worker, world_size=2,
                              timeout=300)
    for r in results:
        assert r == want, (r, want)


def _bloom_tp_save_worker(rank, world_size, path):
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    from alpa_amd.serialization import (model_shard_specs,
                                        save_checkpoint)
    mesh = aa.mesh.full_mesh((1, world_size))
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=32)
    m = BloomModel(cfg, mesh, 1, init_seed=29)
    specs = {f"params.{k}": v
             for k, v in model_shard_specs(m, mesh).items()}
    save_checkpoint(str(path), {"params": dict(m.state_dict())}, 0, specs)
    return True


def test_bloom_tp2_checkpoint_serial_restore(tmp_path):
    """Serving-family checkpoint coverage: BLOOM saved under TP2
    reassembles into the serial layout (Column/Row/Vocab specs apply to
    all decoder families; the non-persistent slope buffer is excluded)."""
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    from alpa_amd.serialization import (model_shard_specs,
                                        restore_checkpoint)
    run_distributed(_bloom_tp_save_worker, world_size=2,
                    args=(str(tmp_path),))
    cfg = BloomConfig(hidden_size=64, num_layers=2, num_heads=4,
                      vocab_size=96, max_seq_len=32)
    m = BloomModel(cfg, None, 1, init_seed=29)
    ref = {n: p.detach().clone() for n, p in m.named_parameters()}
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.0)
    specs = {f"params.{k}": v
             for k, v in model_shard_specs(m).items()}
    restore_checkpoint(str(tmp_path), 0,
                       {"params": dict(m.state_dict())}, specs)
    for n, p in m.named_parameters():
        torch.testing.assert_close(p.detach(), ref[n], rtol=1e-6,
                                   atol=1e-6, msg=lambda msg: f"{n}: {msg}")


def _spmd_serve_worker(rank, world_size):
    from alpa_amd.serve import Controller, SpmdGenerateService
    mesh = aa.mesh.full_mesh((1, world_size))
    m = build_opt(mesh, axis=1)
    svc = SpmdGenerateService(lambda ids, mt: m.generate(ids, mt))
    torch.manual_seed(31)
    ids = torch.randint(0, CFG.vocab_size, (1, 5))
    if rank == 0:
        c = Controller()
        c.register_model("opt", svc)
        out = c.completions("opt", ids.tolist(), max_tokens=4)
        svc.shutdown_workers()
        return out
    svc.serve_worker_loop()
    return None


def test_spmd_serving_tp2():
    """Rank 0 drives the controller; worker ranks execute the same
    generate via broadcast (reference DeviceMeshGroupManager replicas) —
    output equals the serial model."""
    torch.manual_seed(31)
    ids = torch.randint(0, CFG.vocab_size, (1, 5))
    want = build_opt().generate(ids, 4).tolist()
    results = run_distributed(_spmd_serve_worker, world_size=2,
                              timeout=300)
    outs = [r for r in results if r is not None]
    assert len(outs) == 1 and outs[0] == want


def test_continuous_batching_batched_admission_matches_per_request():
    """A burst of >=16 requests into a 16-slot batcher takes the
    BATCHED-prefill admission path (group prefill into contiguous slot
    runs, r2); every request still gets exactly its solo greedy
    tokens."""
    from alpa_amd.serve.batching import ContinuousBatcher, GenRequest
    torch.manual_seed(31)
    m = build_opt()
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, CFG.vocab_size,
                             (int(torch.randint(3, 12, (1,), generator=g)),),
                             generator=g)
               for _ in range(20)]
    want = [m.generate(p.view(1, -1), max_new_tokens=4)[0, len(p):]
            for p in prompts]
    cb = ContinuousBatcher(m, max_batch=16)
    # verify the group path actually engages
    calls = {"n": 0}
    orig = cb._admit_group

    def spy():
        r = orig()
        if r:
            calls["n"] += 1
        return r

    cb._admit_group = spy
    reqs = [GenRequest(p, max_new_tokens=4) for p in prompts]
    for r in reqs:
        cb.submit(r)
    cb.run_all()
    assert calls["n"] >= 1, "batched admission never engaged"
    for r, w in zip(reqs, want):
        assert r.done
        assert r.output == w.tolist(), (r.output, w.tolist())


# ---------------------------------------------------------------------------
# Parameter names are an interface: serve/weights.py and checkpoints address
# them by name.  The lists were recorded from the three separate model files
# before they were folded onto models/decoder.py.
# ---------------------------------------------------------------------------

_STATE_DICT_PINS = {
    "opt": [
        ("blocks.0.fc1.bias", (256,)),
        ("blocks.0.fc1.weight", (256, 64)),
        ("blocks.0.fc2.bias", (64,)),
        ("blocks.0.fc2.weight", (64, 256)),
        ("blocks.0.ln1.bias", (64,)),
        ("blocks.0.ln1.weight", (64,)),
        ("blocks.0.ln2.bias", (64,)),
        ("blocks.0.ln2.weight", (64,)),
        ("blocks.0.out.bias", (64,)),
        ("blocks.0.out.weight", (64, 64)),
        ("blocks.0.qkv.bias", (192,)),
        ("blocks.0.qkv.weight", (192, 64)),
        ("blocks.1.fc1.bias", (256,)),
        ("blocks.1.fc1.weight", (256, 64)),
        ("blocks.1.fc2.bias", (64,)),
        ("blocks.1.fc2.weight", (64, 256)),
        ("blocks.1.ln1.bias", (64,)),
        ("blocks.1.ln1.weight", (64,)),
        ("blocks.1.ln2.bias", (64,)),
        ("blocks.1.ln2.weight", (64,)),
        ("blocks.1.out.bias", (64,)),
        ("blocks.1.out.weight", (64, 64)),
        ("blocks.1.qkv.bias", (192,)),
        ("blocks.1.qkv.weight", (192, 64)),
        ("lm_head.weight", (96, 64)),
        ("ln_f.bias", (64,)),
        ("ln_f.weight", (64,)),
        ("wpe", (66, 64)),
        ("wte.weight", (96, 64)),
    ],
    "bloom": [
        ("blocks.0.fc1.bias", (256,)),
        ("blocks.0.fc1.weight", (256, 64)),
        ("blocks.0.fc2.bias", (64,)),
        ("blocks.0.fc2.weight", (64, 256)),
        ("blocks.0.ln1.bias", (64,)),
        ("blocks.0.ln1.weight", (64,)),
        ("blocks.0.ln2.bias", (64,)),
        ("blocks.0.ln2.weight", (64,)),
        ("blocks.0.out.bias", (64,)),
        ("blocks.0.out.weight", (64, 64)),
        ("blocks.0.qkv.bias", (192,)),
        ("blocks.0.qkv.weight", (192, 64)),
        ("blocks.1.fc1.bias", (256,)),
        ("blocks.1.fc1.weight", (256, 64)),
        ("blocks.1.fc2.bias", (64,)),
        ("blocks.1.fc2.weight", (64, 256)),
        ("blocks.1.ln1.bias", (64,)),
        ("blocks.1.ln1.weight", (64,)),
        ("blocks.1.ln2.bias", (64,)),
        ("blocks.1.ln2.weight", (64,)),
        ("blocks.1.out.bias", (64,)),
        ("blocks.1.out.weight", (64, 64)),
        ("blocks.1.qkv.bias", (192,)),
        ("blocks.1.qkv.weight", (192, 64)),
        ("lm_head.weight", (96, 64)),
        ("ln_emb.bias", (64,)),
        ("ln_emb.weight", (64,)),
        ("ln_f.bias", (64,)),
        ("ln_f.weight", (64,)),
        ("wte.weight", (96, 64)),
    ],
    "codegen": [
        ("blocks.0.fc1.bias", (256,)),
        ("blocks.0.fc1.weight", (256, 64)),
        ("blocks.0.fc2.bias", (64,)),
        ("blocks.0.fc2.weight", (64, 256)),
        ("blocks.0.ln.bias", (64,)),
        ("blocks.0.ln.weight", (64,)),
        ("blocks.0.out.bias", (64,)),
        ("blocks.0.out.weight", (64, 64)),
        ("blocks.0.qkv.bias", (192,)),
        ("blocks.0.qkv.weight", (192, 64)),
        ("blocks.1.fc1.bias", (256,)),
        ("blocks.1.fc1.weight", (256, 64)),
        ("blocks.1.fc2.bias", (64,)),
        ("blocks.1.fc2.weight", (64, 256)),
        ("blocks.1.ln.bias", (64,)),
        ("blocks.1.ln.weight", (64,)),
        ("blocks.1.out.bias", (64,)),
        ("blocks.1.out.weight", (64, 64)),
        ("blocks.1.qkv.bias", (192,)),
        ("blocks.1.qkv.weight", (192, 64)),
        ("lm_head.weight", (96, 64)),
        ("ln_f.bias", (64,)),
        ("ln_f.weight", (64,)),
        ("wte.weight", (96, 64)),
    ],
}


@pytest.mark.parametrize("family", sorted(_STATE_DICT_PINS))
def test_state_dict_names_and_shapes_pinned(family):
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    tiny = dict(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
                max_seq_len=64)
    m = {"opt": build_opt,
         "bloom": lambda: BloomModel(BloomConfig(**tiny), init_seed=19),
         "codegen": lambda: CodeGenModel(
             CodeGenConfig(rotary_dim=8, **tiny), init_seed=17)}[family]()
    got = sorted((k, tuple(v.shape)) for k, v in m.state_dict().items())
    assert got == _STATE_DICT_PINS[family]
    # the non-persistent buffers stay out of the state_dict and stay put
    buffers = {"opt": [], "bloom": ["slopes"],
               "codegen": ["rot_sin", "rot_cos"]}[family]
    assert [n for n, _ in m.named_buffers()] == buffers
