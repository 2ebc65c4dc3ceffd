"""Shared by test_kv_fp8_cpu.py and test_kv_fp8_gpu.py: the elementwise bound
of the e4m3 row format and the tiny decoders of the model tests."""
import torch

# Effect of the e4m3 cache alone on the logits of one cached step after a
# 16-token prefill: max |fp32 CPU model with the reference fp8 cache - its own
# full forward|, seed 0 (the same comparison with a bf16-free fp32 cache gives
# 2e-6).  Measured on the CPU: 0.0543 (CodeGen), 0.0549 (BLOOM).  A test
# allows twice that, 0.109 / 0.110, on top of what it allowed before.
EFFECT = {"codegen": 0.0543, "bloom": 0.0549}
VOCAB = {"codegen": 512, "bloom": 128}


def tiny_model(name, dtype, device):
    """The tiny CodeGen of test_codegen_generation_on_gpu, or a tiny BLOOM
    (ALiBi)."""
    import alpa_amd as aa
    aa.init()
    if name == "codegen":
        from alpa_amd.models.codegen import CodeGenConfig, CodeGenModel
        cfg = CodeGenConfig(hidden_size=256, num_layers=2, num_heads=4,
                            vocab_size=512, max_seq_len=128, rotary_dim=16)
        return CodeGenModel(cfg, None, 1, dtype, device, init_seed=6)
    from alpa_amd.models.bloom import BloomConfig, BloomModel
    cfg = BloomConfig(hidden_size=128, num_layers=2, num_heads=2,
                      vocab_size=128, max_seq_len=32)
    return BloomModel(cfg, None, 1, dtype, device, init_seed=7)


@torch.no_grad()
def cached_step_and_full(m, name):
    """Logits of one cached step after a 16-token prefill, and of the full
    forward over the same 17 tokens."""
    torch.manual_seed(0)
    ids = torch.randint(0, VOCAB[name], (2, 16)).to(m.device_)
    cache = m.new_cache(2)
    nxt = m.greedy_token(m.forward_step(ids, cache)).unsqueeze(1)
    inc = m.forward_step(nxt, cache)
    full = m.forward_step(torch.cat([ids, nxt], 1), m.new_cache(2))
    return inc.float(), full.float()


def check_rows(x, q, scale):
    """|x - scale q| <= max(2^-4 |x|, 2^-10 scale) elementwise, with one
    fp32 ulp of slack: half of e4m3's 3-bit mantissa spacing and half of its
    subnormal spacing.  amax |q| == 448 in every non-zero row, scale == 1 in
    every zero row."""
    x, qf, sc = x.float().cpu(), q.float().cpu(), scale.cpu().unsqueeze(-1)
    bound = torch.maximum(2.0 ** -4 * x.abs(), 2.0 ** -10 * sc)
    assert bool(((x - sc * qf).abs() <= bound * (1 + 2.0 ** -23)).all())
    zero = x.abs().amax(-1) == 0
    assert bool((qf.abs().amax(-1)[~zero] == 448).all())
    assert bool((scale.cpu()[zero] == 1).all())
