"""GPU numerics tests: every gfx950 HIP kernel vs the plain-PyTorch fp32
reference (alpa_amd.ops.reference).  Run on an MI355X via gpurun."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd.ops import reference as ref


@pytest.fixture(scope="module")
def ext():
    from alpa_amd.ops._backend import hip_ops
    e = hip_ops()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def test_mfma_layout_probe(ext):
    """Verify the assumed MFMA 16x16x32 fragment layouts (guide: verify
    with ASYMMETRIC operands — symmetric tests can miss transposes)."""
    torch.manual_seed(0)
    a = torch.randn(16, 32, device="cuda").to(torch.bfloat16)
    b = torch.randn(32, 16, device="cuda").to(torch.bfloat16)
    d = ext.mfma_probe(a.contiguous(), b.contiguous())
    d_ref = a.float() @ b.float()
    torch.testing.assert_close(d, d_ref, rtol=2e-2, atol=2e-2)


def test_layer_norm_fwd_bwd(ext):
    torch.manual_seed(1)
    N, H = 512, 2560
    x = torch.randn(N, H, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(H, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(H, device="cuda", dtype=torch.bfloat16)
    y, mean, rstd = ext.layer_norm_fwd(x, w, b, 1e-5)
    y_ref, mean_ref, rstd_ref = ref.layer_norm_fwd(x.float(), w.float(),
                                                   b.float(), 1e-5)
    torch.testing.assert_close(mean, mean_ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(rstd, rstd_ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(y.float(), y_ref, rtol=2e-2, atol=2e-2)

    dy = torch.randn_like(x)
    dx, dw, db = ext.layer_norm_bwd(dy, x, w, mean, rstd)
    dx_ref, dw_ref, db_ref = ref.layer_norm_bwd(dy.float(), x.float(),
                                                w.float(), mean_ref, rstd_ref)
    torch.testing.assert_close(dx.float(), dx_ref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dw, dw_ref, rtol=2e-2, atol=2e-1)
    torch.testing.assert_close(db, db_ref, rtol=2e-2, atol=2e-1)


def test_bias_gelu_fwd_bwd(ext):
    torch.manual_seed(2)
    N, F = 1024, 10240
    x = torch.randn(N, F, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(F, device="cuda", dtype=torch.bfloat16)
    y = ext.bias_gelu_fwd(x, b)
    y_ref = ref.bias_gelu_fwd(x.float(), b.float())
    torch.testing.assert_close(y.float(), y_ref, rtol=2e-2, atol=2e-2)

    dy = torch.randn_like(x)
    dx, db = ext.bias_gelu_bwd(dy, x, b)
    dx_ref, db_ref = ref.bias_gelu_bwd(dy.float(), x.float(), b.float())
    torch.testing.assert_close(dx.float(), dx_ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(db, db_ref, rtol=2e-2, atol=5e-1)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,D", [(256, 64), (1024, 80), (512, 128),
                                 (192, 80)])
def test_attention_fwd(ext, causal, S, D):
    torch.manual_seed(3)
    B, Hh = 2, 4
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, causal, scale)
    o_ref, lse_ref = ref.attention_fwd(q.float(), k.float(), v.float(),
                                       causal, scale)
    torch.testing.assert_close(o.float(), o_ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.view(-1), lse_ref.view(-1), rtol=1e-3,
                               atol=1e-3)


def test_attention_bwd(ext):
    torch.manual_seed(4)
    B, Hh, S, D = 2, 4, 512, 80
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, True, scale)
    do = torch.randn_like(o)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse.view(B, Hh, S), True, scale)
    dq_r, dk_r, dv_r = ref.attention_bwd(do.float(), q.float(), k.float(),
                                         v.float(), o.float(),
                                         lse.view(B, Hh, S), True, scale)
    torch.testing.assert_close(dq.float(), dq_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk.float(), dk_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv.float(), dv_r, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("S,D,causal", [(1024, 80, True), (256, 64, False),
                                        (512, 128, True), (192, 80, True)])
def test_attention_bwd_fused_vs_blocked(ext, S, D, causal):
    """Hand-written MFMA bwd vs the blocked hipBLASLt reference bwd."""
    torch.manual_seed(11)
    B, Hh = 2, 4
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, causal, scale)
    do = torch.randn_like(o)
    lse3 = lse.view(B, Hh, S)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse3, causal, scale)
    dq_b, dk_b, dv_b = ext.attn_bwd_blocked(do, q, k, v, o, lse3, causal,
                                            scale)
    torch.testing.assert_close(dq.float(), dq_b.float(), rtol=3e-2,
                               atol=3e-2)
    torch.testing.assert_close(dk.float(), dk_b.float(), rtol=3e-2,
                               atol=3e-2)
    torch.testing.assert_close(dv.float(), dv_b.float(), rtol=3e-2,
                               atol=3e-2)


def test_flash_attention_qkv_packed(ext):
    """Packed-qkv strided path (fwd+bwd) vs reference via autograd."""
    from alpa_amd import ops
    torch.manual_seed(7)
    B, S, h, d = 2, 256, 4, 80
    qkv = torch.randn(B, S, h * 3 * d, device="cuda", dtype=torch.bfloat16,
                      requires_grad=True)
    o = ops.flash_attention_qkv(qkv, h, causal=True)
    do = torch.randn_like(o)
    o.backward(do)

    # reference path on fp32 CPU-copy of same math
    qkv5 = qkv.detach().float().view(B, S, h, 3, d)
    q = qkv5[:, :, :, 0].permute(0, 2, 1, 3).contiguous()
    k = qkv5[:, :, :, 1].permute(0, 2, 1, 3).contiguous()
    v = qkv5[:, :, :, 2].permute(0, 2, 1, 3).contiguous()
    o_ref, lse_ref = ref.attention_fwd(q, k, v, True, None)
    o_ref2 = o_ref.permute(0, 2, 1, 3).reshape(B, S, h * d)
    torch.testing.assert_close(o.float(), o_ref2, rtol=2e-2, atol=2e-2)
    dq, dk, dv = ref.attention_bwd(
        do.float().view(B, S, h, d).permute(0, 2, 1, 3).contiguous(), q, k,
        v, o_ref, lse_ref, True, None)
    dqkv_ref = torch.empty(B, S, h, 3, d, device="cuda")
    dqkv_ref[:, :, :, 0] = dq.permute(0, 2, 1, 3)
    dqkv_ref[:, :, :, 1] = dk.permute(0, 2, 1, 3)
    dqkv_ref[:, :, :, 2] = dv.permute(0, 2, 1, 3)
    torch.testing.assert_close(qkv.grad.float(),
                               dqkv_ref.reshape(B, S, h * 3 * d), rtol=4e-2,
                               atol=4e-2)


def test_cross_entropy_fwd_bwd(ext):
    torch.manual_seed(5)
    N, V = 2048, 51200
    logits = torch.randn(N, V, device="cuda", dtype=torch.bfloat16)
    targets = torch.randint(0, V, (N,), device="cuda")
    loss, lse = ext.cross_entropy_fwd(logits, targets)
    loss_ref, lse_ref = ref.softmax_cross_entropy_fwd(logits.float(), targets)
    torch.testing.assert_close(loss, loss_ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse, lse_ref, rtol=1e-3, atol=1e-3)

    dloss = torch.randn(N, device="cuda")
    dlogits = ext.cross_entropy_bwd(dloss, logits, targets, lse)
    dl_ref = ref.softmax_cross_entropy_bwd(dloss, logits.float(), targets,
                                           lse_ref)
    torch.testing.assert_close(dlogits.float(), dl_ref, rtol=2e-2, atol=2e-2)


def test_adamw_fused(ext):
    """Full python-wrapper path vs fp32 reference."""
    from alpa_amd import ops
    torch.manual_seed(6)
    shapes = [(1000, 33), (4097,), (128, 256)]
    params = [torch.randn(s, device="cuda", dtype=torch.bfloat16)
              for s in shapes]
    grads = [torch.randn(s, device="cuda", dtype=torch.bfloat16)
             for s in shapes]
    ms = [torch.zeros(s, device="cuda") for s in shapes]
    vs = [torch.zeros(s, device="cuda") for s in shapes]

    p_ref = [p.float().clone() for p in params]
    g_ref = [g.float() for g in grads]
    m_ref = [m.clone() for m in ms]
    v_ref = [v.clone() for v in vs]

    for step in (1, 2, 3):
        ops.fused_adamw(params, grads, ms, vs, step, lr=1e-2, beta1=0.9,
                        beta2=0.95, eps=1e-8, weight_decay=0.1,
                        grad_scale=0.5)
        ref.adamw_step(p_ref, g_ref, m_ref, v_ref, step, lr=1e-2, beta1=0.9,
                       beta2=0.95, eps=1e-8, weight_decay=0.1, grad_scale=0.5)
    for p, pr in zip(params, p_ref):
        # bf16 params accumulate rounding each step vs fp32 ref
        torch.testing.assert_close(p.float(), pr, rtol=2e-2, atol=2e-2)
    for m, mr in zip(ms, m_ref):
        torch.testing.assert_close(m, mr, rtol=1e-2, atol=1e-3)


def test_gpt_step_on_gpu():
    """Whole-model smoke through the HIP kernel path."""
    import alpa_amd as aa
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    aa.init()
    cfg = GPTConfig(hidden_size=256, num_layers=2, num_heads=4, seq_len=128,
                    vocab_size=1024)
    method = aa.ShardParallel(logical_mesh_shape=(1, 1))

    def build(mesh=None, axis=1, dtype=torch.bfloat16, device=None):
        torch.manual_seed(0)
        return GPTModel(cfg, mesh, axis, dtype, device)

    state = aa.TrainState.create(build, method, lr=1e-3)
    step = aa.parallelize(lambda m, b: m.loss(b[0], b[1]), method=method)
    ids = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len), device="cuda")
    labels = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len), device="cuda")
    losses = [float(step(state, (ids, labels))) for _ in range(6)]
    assert all(l == l for l in losses), f"NaN in {losses}"
    assert losses[-1] < losses[0], losses


def test_moe_gpt_step_on_gpu():
    """MoE model single-GPU smoke through the HIP kernel path."""
    import alpa_amd as aa
    from alpa_amd.models.moe import MoEConfig, MoEGPTModel
    aa.init()
    cfg = MoEConfig(hidden_size=256, num_layers=2, num_heads=4, seq_len=128,
                    vocab_size=1024, num_experts=4, moe_every=2)
    method = aa.ShardParallel(logical_mesh_shape=(1, 1))

    def build(mesh=None, axis=1, dtype=torch.bfloat16, device=None):
        return MoEGPTModel(cfg, mesh, axis, dtype, device, init_seed=2)

    state = aa.TrainState.create(build, method, lr=1e-3)
    step = aa.parallelize(lambda m, b: m.loss(b[0], b[1]), method=method)
    ids = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len), device="cuda")
    labels = torch.randint(0, cfg.vocab_size, (4, cfg.seq_len), device="cuda")
    losses = [float(step(state, (ids, labels))) for _ in range(6)]
    assert all(l == l for l in losses), f"NaN in {losses}"
    assert losses[-1] < losses[0], losses


def test_add_layer_norm_fused(ext):
    """Fused residual-add + LN vs reference."""
    torch.manual_seed(12)
    N, H = 512, 2560
    a = torch.randn(N, H, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(N, H, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(H, device="cuda", dtype=torch.bfloat16)
    bias = torch.randn(H, device="cuda", dtype=torch.bfloat16)
    h, y, mean, rstd = ext.add_layer_norm_fwd(a, b, w, bias, 1e-5)
    h_ref = (a.float() + b.float())
    torch.testing.assert_close(h.float(), h_ref, rtol=2e-2, atol=2e-2)
    y_ref, mean_ref, rstd_ref = ref.layer_norm_fwd(h.float(), w.float(),
                                                   bias.float(), 1e-5)
    torch.testing.assert_close(y.float(), y_ref, rtol=2e-2, atol=2e-2)

    dy = torch.randn_like(y)
    dh = torch.randn_like(y)
    dx, dw, db = ext.add_layer_norm_bwd(dy, dh, h, w, mean, rstd)
    dx_ref, dw_ref, db_ref = ref.layer_norm_bwd(dy.float(), h.float(),
                                                w.float(), mean_ref,
                                                rstd_ref)
    torch.testing.assert_close(dx.float(), dx_ref + dh.float(), rtol=3e-2,
                               atol=3e-2)
    torch.testing.assert_close(dw, dw_ref, rtol=2e-2, atol=2e-1)
    torch.testing.assert_close(db, db_ref, rtol=2e-2, atol=2e-1)


def test_opt_generation_on_gpu():
    """Serving path on GPU: prefill + strided-KV-cache decode through the
    attention kernel."""
    import alpa_amd as aa
    from alpa_amd.models.opt import OPTConfig, OPTModel
    aa.init()
    cfg = OPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                    vocab_size=512, max_seq_len=128)
    m = OPTModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=4)
    ids = torch.randint(0, 512, (2, 16), device="cuda")
    out = m.generate(ids, max_new_tokens=8)
    assert out.shape == (2, 24)
    # cache decode must equal full recompute
    cache = m.new_cache(2)
    logits_inc = m.forward_step(ids, cache)
    nxt = m.greedy_token(logits_inc).unsqueeze(1)
    logits_inc = m.forward_step(nxt, cache)
    cache2 = m.new_cache(2)
    logits_full = m.forward_step(torch.cat([ids, nxt], 1), cache2)
    torch.testing.assert_close(logits_inc.float(), logits_full.float(),
                               rtol=5e-2, atol=5e-2)
    # beam search: KV-cache reorder between steps on device
    beam = m.beam_search(ids, max_new_tokens=6, num_beams=3, eos_token=2)
    assert beam.shape[0] == 2 and beam.shape[1] <= 22
    assert beam.is_cuda


def test_bert_and_unet_on_gpu():
    from alpa_amd.models.bert import BertConfig, BertModel
    from alpa_amd.models.unet import UNet2D
    cfg = BertConfig(hidden_size=128, num_layers=2, num_heads=4, seq_len=64,
                     vocab_size=512)
    bert = BertModel(cfg, dtype=torch.bfloat16, device="cuda", init_seed=3)
    ids = torch.randint(0, 512, (2, 64), device="cuda")
    loss = bert.mlm_loss(ids, ids)
    loss.backward()
    assert float(loss) == float(loss)

    unet = UNet2D(in_ch=3, base=16, ch_mults=(1, 2), dtype=torch.bfloat16,
                  device="cuda")
    x = torch.randn(2, 3, 16, 16, device="cuda", dtype=torch.bfloat16)
    t = torch.randint(0, 1000, (2,), device="cuda")
    loss = unet.loss(x, t, torch.randn_like(x))
    loss.backward()
    assert float(loss) == float(loss)

    from alpa_amd.models.vit import ViTConfig, ViTModel
    vcfg = ViTConfig(image_size=64, patch_size=16, hidden_size=128,
                     num_layers=2, num_heads=4, num_classes=10)
    vit = ViTModel(vcfg, dtype=torch.bfloat16, device="cuda", init_seed=2)
    img = torch.randn(2, 3, 64, 64, device="cuda", dtype=torch.bfloat16)
    loss = vit.loss(img, torch.randint(0, 10, (2,), device="cuda"))
    loss.backward()
    assert float(loss) == float(loss)


def test_zero_paths_single_gpu():
    """ZeRO-2/3 optimizer paths through the fused kernels (dp=1 degenerate:
    no collectives, but the shard/gather bookkeeping runs)."""
    import alpa_amd as aa
    from alpa_amd.testing import MLPModel
    aa.init()
    for method in (aa.Zero2Parallel(num_micro_batches=2),
                   aa.Zero3Parallel(num_micro_batches=2)):
        def build(mesh=None, axis=1, dtype=torch.bfloat16, device=None):
            return MLPModel(hidden=128, mesh=mesh, axis=axis, dtype=dtype,
                            device=device)
        state = aa.TrainState.create(build, method, lr=1e-3)
        step = aa.parallelize(lambda m, b: m.loss(*b), method=method)
        x = torch.randn(4, 128, device="cuda", dtype=torch.bfloat16)
        y = torch.randn(4, 128, device="cuda", dtype=torch.bfloat16)
        first = float(step(state, (x, y)))
        for _ in range(4):
            last = float(step(state, (x, y)))
        assert last < first, (type(method).__name__, first, last)


def test_mfma32_layout_probe(ext):
    """Verify the 32x32x16 fragment layouts with asymmetric operands."""
    torch.manual_seed(13)
    a = torch.randn(32, 16, device="cuda").to(torch.bfloat16)
    b = torch.randn(16, 32, device="cuda").to(torch.bfloat16)
    d = ext.mfma_probe32(a.contiguous(), b.contiguous())
    d_ref = a.float() @ b.float()
    torch.testing.assert_close(d, d_ref, rtol=2e-2, atol=2e-2)


def test_ring_attention_chunk_decomposition(ext):
    """Ring attention on GPU decomposes full attention into per-KV-chunk
    kernel calls merged via the kernel-emitted lse (parallel/
    ring_attention.py); single-device check: 2 chunk calls + lse merge ==
    one full-sequence call, fwd AND bwd."""
    from alpa_amd.parallel.ring_attention import _merge
    torch.manual_seed(12)
    B, Hh, S, D = 2, 4, 512, 64
    half = S // 2
    scale = 1.0 / math.sqrt(D)
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    o_full, lse_full = ext.attn_fwd(q, k, v, False, scale)
    # fwd: q vs kv-chunk0 and q vs kv-chunk1, merged
    o0, lse0 = ext.attn_fwd(q, k[:, :, :half].contiguous(),
                            v[:, :, :half].contiguous(), False, scale)
    o1, lse1 = ext.attn_fwd(q, k[:, :, half:].contiguous(),
                            v[:, :, half:].contiguous(), False, scale)
    o_m, lse_m = _merge(o0.float(), lse0.view(B, Hh, S).float(),
                        o1, lse1.view(B, Hh, S).float())
    torch.testing.assert_close(o_m, o_full.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse_m, lse_full.view(B, Hh, S).float(),
                               rtol=1e-3, atol=1e-3)
    # bwd: per-chunk calls with the GLOBAL o/lse sum to the full grads
    do = torch.randn_like(o_full)
    dq_f, dk_f, dv_f = ext.attn_bwd(do, q, k, v, o_full,
                                    lse_full.view(B, Hh, S), False, scale)
    lse_g = lse_full.view(B, Hh, S)
    dq0, dk0, dv0 = ext.attn_bwd(do, q, k[:, :, :half].contiguous(),
                                 v[:, :, :half].contiguous(), o_full,
                                 lse_g, False, scale)
    dq1, dk1, dv1 = ext.attn_bwd(do, q, k[:, :, half:].contiguous(),
                                 v[:, :, half:].contiguous(), o_full,
                                 lse_g, False, scale)
    torch.testing.assert_close((dq0.float() + dq1.float()), dq_f.float(),
                               rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(torch.cat([dk0, dk1], 2).float(),
                               dk_f.float(), rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(torch.cat([dv0, dv1], 2).float(),
                               dv_f.float(), rtol=3e-2, atol=3e-2)


def test_codegen_generation_on_gpu():
    """Rotary decoder (CodeGen) prefill + cached decode on the gfx950
    attention kernel."""
    import alpa_amd as aa
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    aa.init()
    cfg = CodeGenConfig(hidden_size=256, num_layers=2, num_heads=4,
                        vocab_size=512, max_seq_len=128, rotary_dim=16)
    m = CodeGenModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=6)
    ids = torch.randint(0, 512, (2, 16), device="cuda")
    out = m.generate(ids, max_new_tokens=8)
    assert out.shape == (2, 24)
    cache = m.new_cache(2)
    logits_inc = m.forward_step(ids, cache)
    nxt = m.greedy_token(logits_inc).unsqueeze(1)
    logits_inc = m.forward_step(nxt, cache)
    logits_full = m.forward_step(torch.cat([ids, nxt], 1), m.new_cache(2))
    torch.testing.assert_close(logits_inc.float(), logits_full.float(),
                               rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("causal,S,Skv", [(True, 512, 512),
                                          (False, 1, 257)])
def test_attention_alibi_fwd(ext, causal, S, Skv):
    """ALiBi bias inside the fwd kernel vs the fp32 reference — training
    (square causal) and cached-decode (S=1, q offset Skv-S) shapes."""
    from alpa_amd.models.bloom import alibi_slopes
    torch.manual_seed(14)
    B, Hh, D = 2, 4, 64
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    slopes = alibi_slopes(Hh).cuda()
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, causal, scale, slopes)
    o_r, lse_r = ref.attention_fwd(q.float(), k.float(), v.float(), causal,
                                   scale, slopes)
    torch.testing.assert_close(o.float(), o_r, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.view(-1), lse_r.view(-1), rtol=1e-3,
                               atol=1e-3)


def test_attention_alibi_bwd(ext):
    from alpa_amd.models.bloom import alibi_slopes
    torch.manual_seed(15)
    B, Hh, S, D = 2, 4, 512, 64
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    slopes = alibi_slopes(Hh).cuda()
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, True, scale, slopes)
    do = torch.randn_like(o)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse.view(B, Hh, S), True,
                              scale, slopes)
    dq_r, dk_r, dv_r = ref.attention_bwd(
        do.float(), q.float(), k.float(), v.float(), o.float(),
        lse.view(B, Hh, S), True, scale, slopes)
    torch.testing.assert_close(dq.float(), dq_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dk.float(), dk_r, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dv.float(), dv_r, rtol=3e-2, atol=3e-2)


def test_bloom_generation_on_gpu():
    """ALiBi decoder (BLOOM) prefill + cached decode with the in-kernel
    bias."""
    import alpa_amd as aa
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    aa.init()
    cfg = BloomConfig(hidden_size=256, num_layers=2, num_heads=4,
                      vocab_size=512, max_seq_len=128)
    m = BloomModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=7)
    ids = torch.randint(0, 512, (2, 16), device="cuda")
    out = m.generate(ids, max_new_tokens=8)
    assert out.shape == (2, 24)
    cache = m.new_cache(2)
    logits_inc = m.forward_step(ids, cache)
    nxt = m.greedy_token(logits_inc).unsqueeze(1)
    logits_inc = m.forward_step(nxt, cache)
    logits_full = m.forward_step(torch.cat([ids, nxt], 1), m.new_cache(2))
    torch.testing.assert_close(logits_inc.float(), logits_full.float(),
                               rtol=5e-2, atol=5e-2)


def test_bloom_per_slot_decode_on_gpu():
    """BLOOM through forward_decode (continuous batching): two slots at
    unequal lengths decode in one varlen call with slopes; each slot's
    logits match that slot decoded alone through forward_step.  Same
    tolerance as test_bloom_generation_on_gpu."""
    import alpa_amd as aa
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    from alpa_amd.serve.batching import _SlotCacheView
    aa.init()
    cfg = BloomConfig(hidden_size=128, num_layers=2, num_heads=2,
                      vocab_size=128, max_seq_len=32)
    m = BloomModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=7)
    torch.manual_seed(20)
    lens = torch.tensor([5, 8], device="cuda")
    cache = m.new_cache(2)
    views, cur = [], []
    with torch.no_grad():
        for b, n in enumerate(lens.tolist()):
            views.append(_SlotCacheView(cache, b))
            ids = torch.randint(0, 128, (1, n), device="cuda")
            cur.append(m.greedy_token(m.forward_step(ids, views[b])))
        cur = torch.stack(cur)                       # [2, 1]
        logits = m.forward_decode(cur, cache, lens)
        for b in range(2):
            solo = m.forward_step(cur[b:b + 1], views[b])
            torch.testing.assert_close(logits[b:b + 1].float(),
                                       solo.float(), rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_attention_one_visible_key(D):
    """One query, one key: the softmax weight is exactly 1, so o is v bit
    for bit on every route flash_attention takes — causal (prefill kernel;
    the blocked path at D=256) and non-causal (split-KV decode kernel).
    This is what lets the cached decoders use causal = S > 1 for a
    one-token prompt."""
    from alpa_amd import ops
    torch.manual_seed(21)
    q, k, v = (torch.randn(2, 2, 1, D, device="cuda", dtype=torch.bfloat16)
               for _ in range(3))
    assert torch.equal(ops.flash_attention(q, k, v, causal=True), v)
    assert torch.equal(ops.flash_attention(q, k, v, causal=False), v)


def test_attention_varlen_gpu(ext):
    """Per-batch kv_lens masking in the fwd kernel vs per-request
    separate kernel calls."""
    torch.manual_seed(16)
    B, Hh, D, Skv = 4, 4, 64, 257
    q = torch.randn(B, Hh, 1, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, Skv, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    lens = torch.tensor([3, 257, 100, 64], dtype=torch.int32,
                        device="cuda")
    o, _ = ext.attn_fwd(q, k, v, False, scale, None, lens)
    for b, L in enumerate(lens.tolist()):
        ob, _ = ext.attn_fwd(q[b:b + 1].contiguous(),
                             k[b:b + 1, :, :L].contiguous(),
                             v[b:b + 1, :, :L].contiguous(), False, scale)
        torch.testing.assert_close(o[b:b + 1].float(), ob.float(),
                                   rtol=2e-2, atol=2e-2)


def test_continuous_batching_on_gpu():
    """Slot batcher end-to-end on the varlen kernel."""
    import alpa_amd as aa
    from alpa_amd.models.opt import OPTConfig, OPTModel
    from alpa_amd.serve.batching import ContinuousBatcher, GenRequest
    aa.init()
    cfg = OPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                    vocab_size=512, max_seq_len=128)
    m = OPTModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=4)
    torch.manual_seed(17)
    prompts = [torch.randint(0, 512, (n,)) for n in (5, 9, 3)]
    want = [m.generate(p.view(1, -1).cuda(), max_new_tokens=5)[0, len(p):]
            for p in prompts]
    cb = ContinuousBatcher(m, max_batch=2)
    reqs = [GenRequest(p, max_new_tokens=5) for p in prompts]
    for r in reqs:
        cb.submit(r)
    cb.run_all()
    for r, w in zip(reqs, want):
        assert r.done and r.output == w.tolist(), (r.output, w.tolist())


def test_attention_fwd_blocked_d256(ext):
    """head_dim 256 (CodeGen-6B/16B class) via the blocked hipBLASLt
    path vs fp32 reference — prefill (causal) and decode shapes."""
    torch.manual_seed(18)
    B, Hh, S, D = 2, 2, 256, 256
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd_blocked(q, k, v, True, scale)
    o_r, lse_r = ref.attention_fwd(q.float(), k.float(), v.float(), True,
                                   scale)
    torch.testing.assert_close(o.float(), o_r, rtol=2e-2, atol=2e-2)
    # scores come from bf16-input GEMMs: 256-term dots carry ~1e-2 noise
    torch.testing.assert_close(lse.view(-1), lse_r.view(-1), rtol=1e-2,
                               atol=1e-2)
    # decode shape: 1 query vs 129-entry cache
    q1 = q[:, :, :1].contiguous()
    k1 = k[:, :, :129].contiguous()
    v1 = v[:, :, :129].contiguous()
    o, lse = ext.attn_fwd_blocked(q1, k1, v1, False, scale)
    o_r, _ = ref.attention_fwd(q1.float(), k1.float(), v1.float(), False,
                               scale)
    torch.testing.assert_close(o.float(), o_r, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,D", [(192, 256), (192, 160)])
def test_attention_fwd_fused_d256(ext, causal, S, D):
    """The fused single-buffered Dp=256 forward (head_dim in (128, 256]).
    S=192 is one full 128-row block plus a ragged one over three 64-wide
    kv tiles; D=160 exercises the head-dim guards inside Dp=256.  Same
    bounds as test_attention_fwd: both kernels accumulate scores in fp32
    from the same bf16 inputs."""
    torch.manual_seed(19)
    B, Hh = 1, 2
    q = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hh, S, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, causal, scale)
    o_ref, lse_ref = ref.attention_fwd(q.float(), k.float(), v.float(),
                                       causal, scale)
    torch.testing.assert_close(o.float(), o_ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.view(-1), lse_ref.view(-1), rtol=1e-3,
                               atol=1e-3)


def test_codegen_6b_heads_on_gpu():
    """A CodeGen-6B-shaped decoder (head_dim 256) generates end-to-end
    through the blocked attention path."""
    import alpa_amd as aa
    from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
    aa.init()
    cfg = CodeGenConfig(hidden_size=1024, num_layers=2, num_heads=4,
                        vocab_size=512, max_seq_len=128, rotary_dim=64)
    assert cfg.head_dim == 256
    m = CodeGenModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=8)
    ids = torch.randint(0, 512, (2, 12), device="cuda")
    out = m.generate(ids, max_new_tokens=6)
    assert out.shape == (2, 18)


def test_fp8_linear_numerics():
    """fp8 GEMM recipe (ops/fp8.py, round 2: fwd AND bwd fp8 with
    delayed scaling): forward within fp8 quantization error of bf16;
    backward grads within the e4m3 tolerance."""
    from alpa_amd.ops.fp8 import fp8_available, fp8_linear
    torch.manual_seed(19)
    x = torch.randn(512, 1024, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    w = torch.randn(2048, 1024, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True) * 0.02
    w.retain_grad()
    assert fp8_available(x)
    b = torch.randn(2048, device="cuda", dtype=torch.bfloat16)

    class Anchor(torch.nn.Module):
        pass

    y = fp8_linear(x, w, b, module=Anchor().cuda())
    ref = torch.nn.functional.linear(x, w, b)
    rel = (y.float() - ref.float()).abs().mean() / ref.float().abs().mean()
    assert rel < 0.06, float(rel)
    dy = torch.randn_like(y)
    y.backward(dy)
    dx_ref = dy @ w
    rel = (x.grad.float() - dx_ref.float()).abs().mean() / \
        dx_ref.float().abs().mean()
    assert rel < 0.06, float(rel)


def test_fp8_gpt_step():
    """GPT step with fp8-forward projections runs end to end and the
    loss stays finite (opt-in global_config.fp8_gemm)."""
    import alpa_amd as aa
    from alpa_amd.global_env import global_config
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    aa.init()
    cfg = GPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                    seq_len=128, vocab_size=1024)
    m = GPTModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=3)
    ids = torch.randint(0, 1024, (4, 128), device="cuda")
    global_config.fp8_gemm = True
    try:
        loss = m.loss(ids, ids)
        loss.backward()
        assert float(loss) == float(loss)
        loss_bf16_grad = [p.grad.abs().sum().item()
                          for p in list(m.parameters())[:3]]
        assert all(g == g for g in loss_bf16_grad)
    finally:
        global_config.fp8_gemm = False


def test_moe_scale_regression():
    """Pin the hipBLASLt bmm-backward fault workaround: the expert FFN
    at realistic MoE scale (this exact config reproduced
    hipErrorIllegalAddress through torch.bmm backward) must train."""
    from alpa_amd.parallel.expert import ExpertParallelMLP
    torch.manual_seed(24)
    m = ExpertParallelMLP(1024, 4096, 8, None, 1, capacity_factor=2.0,
                          dtype=torch.bfloat16, device="cuda")
    x = torch.randn(16, 1024, 1024, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = m(x)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and float(x.grad.abs().sum()) > 0


def test_colsum_matches_reference():
    """Striped column sum vs fp32 reference (bias-grad path)."""
    torch.manual_seed(4)
    g = (torch.randn(4096, 2560, device="cuda") * 2).to(torch.bfloat16)
    from alpa_amd.ops._backend import hip_ops
    got = hip_ops().colsum_bf16(g.contiguous())
    ref = g.float().sum(0)
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-1)


def test_bias_add_backward_matches():
    from alpa_amd import ops
    x = torch.randn(512, 33, 768, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    b = torch.randn(768, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = ops.bias_add(x, b)
    gy = torch.randn_like(y)
    y.backward(gy)
    xr = x.detach().clone().requires_grad_(True)
    br = b.detach().clone().requires_grad_(True)
    (xr + br).backward(gy)
    torch.testing.assert_close(x.grad, xr.grad)
    torch.testing.assert_close(b.grad.float(), br.grad.float(),
                               rtol=1e-2, atol=1e-1)
