"""Producer-fused fp8 quantize on hardware (ops/csrc/fp8_fused.hip).

The yardstick is always the existing two-kernel pipeline: the LayerNorm or
bias+GeLU forward kernel followed by the dual-layout quantize kernel.  The
fused kernels promise its bytes, so every op-level comparison is exact,
NaN codes included.  The function- and model-level comparisons allow what
two runs of the unfused path differ by among themselves (zero when the
library GEMMs are reproducible)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5

# (64, 64) one interior tile; (100, 200) ragged both ways; (1, 8) minimal;
# (17, 2560) two column passes of the 256x8 row loop and a row count that
# is no multiple of the 16-row group; (130, 72) ragged, F % 16 != 0
SHAPES = [(64, 64), (100, 200), (1, 8), (17, 2560), (130, 72)]
# mid-range for randn*3, and one at which most elements clamp at +-448
SCALES = [0.02, 1e-4]


def _ext():
    from alpa_amd.ops._backend import hip_ops
    return hip_ops()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _bytes(t):
    """The tensor's bit patterns: NaNs and signed zeros compare too."""
    return t.view(_BITS[t.dtype.itemsize])


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(_bytes(got), _bytes(want)), what


def _gelu_pair(x, bias, scale):
    ext = _ext()
    y = ext.bias_gelu_fwd(x, bias)
    return ext.fp8_quantize(y.reshape(-1, y.shape[-1]), scale, True, False)


def _check_gelu(x, bias, scale):
    from alpa_amd import ops
    q, qt, amax = ops.bias_gelu_fp8(x, bias, scale)
    q0, qt0, amax0 = _gelu_pair(x, bias, scale)
    _same_bytes(q, q0, "q")
    _same_bytes(qt, qt0, "qt")
    _same_bytes(amax, amax0, "amax")


def _check_ln(a, delta, w, b, scale):
    from alpa_amd import ops
    ext = _ext()
    h, mean, rstd, q, qt, amax = ops.add_layer_norm_fp8(a, delta, w, b, EPS,
                                                        scale)
    h0, y0, mean0, rstd0 = ext.add_layer_norm_fwd(a, delta, w, b, EPS)
    q0, qt0, amax0 = ext.fp8_quantize(y0, scale, True, False)
    _same_bytes(h, h0, "h")
    _same_bytes(mean, mean0, "mean")
    _same_bytes(rstd, rstd0, "rstd")
    _same_bytes(q, q0, "q")
    _same_bytes(qt, qt0, "qt")
    _same_bytes(amax, amax0, "amax")


def _rand(shape, seed):
    g = _gen(seed)
    n, f = shape
    x = (torch.randn(n, f, device="cuda", generator=g) * 3).to(BF16)
    d = torch.randn(n, f, device="cuda", generator=g).to(BF16)
    w = (1 + 0.1 * torch.randn(f, device="cuda", generator=g)).to(BF16)
    b = (0.1 * torch.randn(f, device="cuda", generator=g)).to(BF16)
    return x, d, w, b


# ------------------------------------------------------------------ op level

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_bias_gelu_fp8_bytes(shape, scale):
    x, _, _, b = _rand(shape, 10)
    s = torch.tensor([scale], device="cuda")
    _check_gelu(x, b, s)
    if scale == SCALES[1]:
        q = _ext().bias_gelu_fp8(x, b, s)[0].float().abs()
        if x.numel() >= 64:
            assert (q == 448).float().mean().item() > 0.25, "few clamps"


# the widest row the LayerNorm kernel takes (64 KB of LDS), two row groups
LN_SHAPES = SHAPES + [(20, 4096)]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_add_layer_norm_fp8_bytes(shape, with_delta, scale):
    x, d, w, b = _rand(shape, 11)
    s = torch.tensor([scale], device="cuda")
    _check_ln(x, d if with_delta else None, w, b, s)
    if scale == SCALES[1] and x.numel() >= 64:
        q = _ext().add_layer_norm_fp8(x, None, w, b, EPS, s)[3].float().abs()
        assert (q == 448).float().mean().item() > 0.25, "few clamps"


def _hostile(kind, shape=(33, 200)):
    x, d, w, b = _rand(shape, 12)
    if kind == "const":
        x[5] = 3e4
        d[5] = 0
    elif kind == "inf":
        x[7, 3] = float("inf")
        x[9, 11] = float("-inf")
    elif kind == "zero":
        x.zero_()
        d.zero_()
    return x, d, w, b


@pytest.mark.parametrize("kind", ["const", "inf", "zero"])
def test_hostile_rows_keep_the_bytes(kind):
    """A constant row of 3e4, rows holding +-inf (NaN codes after the
    LayerNorm, and after gelu(-inf)), an all-zero input."""
    x, d, w, b = _hostile(kind)
    s = torch.tensor([0.02], device="cuda")
    _check_gelu(x, b, s)
    _check_ln(x, d, w, b, s)
    _check_ln(x, None, w, b, s)
    if kind == "zero":
        zb = torch.zeros_like(b)
        _check_gelu(x, zb, s)
        q, _, amax = _ext().bias_gelu_fp8(x, zb, s)
        assert amax.item() == 0 and not q.view(torch.uint8).any()


def test_binding_input_checks():
    ext = _ext()
    x, d, w, b = _rand((16, 64), 13)
    s = torch.tensor([0.02], device="cuda")
    with pytest.raises(RuntimeError, match="bf16"):
        ext.bias_gelu_fp8(x.float(), b, s)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.bias_gelu_fp8(x.t(), b, s)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.bias_gelu_fp8(x[:, :60].contiguous(), b[:60].contiguous(), s)
    with pytest.raises(RuntimeError, match="elements"):
        ext.bias_gelu_fp8(x, b[:32].contiguous(), s)
    with pytest.raises(RuntimeError, match="scale"):
        ext.bias_gelu_fp8(x, b, s.cpu())
    with pytest.raises(RuntimeError, match="scale"):
        ext.add_layer_norm_fp8(x, d, w, b, EPS, torch.ones(2, device="cuda"))
    with pytest.raises(RuntimeError, match="shape"):
        ext.add_layer_norm_fp8(x, d[:8].contiguous(), w, b, EPS, s)
    from alpa_amd.ops import ADD_LAYER_NORM_FP8_MAX_H
    wide = torch.zeros(2, ADD_LAYER_NORM_FP8_MAX_H + 8, device="cuda",
                       dtype=BF16)
    with pytest.raises(RuntimeError, match="H <= 4096"):
        ext.add_layer_norm_fp8(wide, None, wide[0].clone(), wide[0].clone(),
                               EPS, s)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.add_layer_norm_fp8(x[:, :60].contiguous(), None,
                               w[:60].contiguous(), b[:60].contiguous(), EPS,
                               s)


# ------------------------------------------------------------ function level

M, H, F = 256, 128, 512


class _Anchor(torch.nn.Module):
    pass


def _clone_anchor(src):
    """A fresh anchor with identical copies of src's delayed-scaling state
    (and no cached weight: every run quantizes it from the same state)."""
    from alpa_amd.ops.fp8 import _RoleState
    dst = _Anchor()
    for name in ("x", "g", "w"):
        st = getattr(src, f"_fp8_{name}", None)
        if st is not None:
            c = _RoleState()
            c.running, c.scale = st.running.clone(), st.scale.clone()
            setattr(dst, f"_fp8_{name}", c)
    return dst


def _state_of(mod):
    out = {}
    for name in ("x", "g", "w"):
        st = getattr(mod, f"_fp8_{name}")
        out[name + ".running"] = st.running.clone()
        out[name + ".scale"] = st.scale.clone()
    return out


def _max_diff(a, b):
    return (a.double() - b.double()).abs().max().item()


def _compare_runs(run_ref, run_new, seed_anchor):
    """run_*(anchor) -> dict of tensors.  The unfused side runs twice from
    identical state; their largest element-wise difference per tensor is
    what the fused side may differ by."""
    r1 = run_ref(_clone_anchor(seed_anchor))
    r2 = run_ref(_clone_anchor(seed_anchor))
    got = run_new(_clone_anchor(seed_anchor))
    assert got.keys() == r1.keys()
    for k in r1:
        tol = _max_diff(r1[k], r2[k])
        diff = _max_diff(got[k], r1[k])
        print(f"{k}: fused-vs-unfused {diff:.3g}, unfused run-to-run "
              f"{tol:.3g}")
        assert got[k].shape == r1[k].shape and got[k].dtype == r1[k].dtype
        assert torch.isfinite(got[k].float()).all(), k
        assert diff <= tol, (k, diff, tol)


@pytest.fixture
def wgrad_on():
    from alpa_amd.global_env import global_config
    old = (global_config.fp8_wgrad, global_config.fp8_dx_bf16)
    global_config.fp8_wgrad, global_config.fp8_dx_bf16 = True, False
    yield
    global_config.fp8_wgrad, global_config.fp8_dx_bf16 = old


@pytest.mark.parametrize("with_delta", [True, False])
def test_fp8_ln_linear_matches_unfused(wgrad_on, with_delta, monkeypatch):
    from alpa_amd import ops
    from alpa_amd.ops.fp8 import fp8_linear, fp8_ln_linear
    g = _gen(20)

    def leaf(*shape, mul=1.0, add=0.0):
        t = torch.randn(*shape, device="cuda", generator=g) * mul + add
        return t.to(BF16).requires_grad_(True)

    res, delta = leaf(M, H), leaf(M, H)
    lnw, lnb = leaf(H, mul=0.1, add=1.0), leaf(H, mul=0.1)
    w, bias = leaf(F, H, mul=0.05), leaf(F, mul=0.1)
    dout = torch.randn(M, F, device="cuda", generator=g).to(BF16)
    dh = torch.randn(M, H, device="cuda", generator=g).to(BF16)
    leaves = {"res": res, "ln_w": lnw, "ln_b": lnb, "w": w, "bias": bias}
    if with_delta:
        leaves["delta"] = delta
    dl = delta if with_delta else None

    def finish(mod, h, out):
        # h also feeds the residual stream: give it a gradient of its own
        grads = torch.autograd.grad([out, h], list(leaves.values()),
                                    [dout, dh])
        r = {"out": out.detach(), "h": h.detach()}
        r.update({"d" + k: v for k, v in zip(leaves, grads)})
        r.update(_state_of(mod))
        return r

    def unfused(mod):
        h, y = ops.add_layer_norm(res, dl, lnw, lnb, EPS)
        return finish(mod, h, fp8_linear(y, w, bias, module=mod))

    calls = []
    real = ops.add_layer_norm_fp8
    monkeypatch.setattr(ops, "add_layer_norm_fp8",
                        lambda *a: calls.append(1) or real(*a))

    def fused(mod):
        h, out = fp8_ln_linear(res, dl, lnw, lnb, EPS, w, bias, mod)
        return finish(mod, h, out)

    seed = _Anchor()
    unfused(seed)                      # gives every role its first scale
    _compare_runs(unfused, fused, seed)
    assert len(calls) == 1, "the fused kernel was not on the path"
    # a module without a scale yet takes the unfused composition
    fresh = fused(_Anchor())
    assert len(calls) == 1 and torch.isfinite(fresh["out"].float()).all()


def test_fp8_gelu_linear_matches_unfused(wgrad_on, monkeypatch):
    from alpa_amd import ops
    from alpa_amd.ops.fp8 import fp8_gelu_linear, fp8_linear
    g = _gen(21)

    def leaf(*shape, mul=1.0):
        t = torch.randn(*shape, device="cuda", generator=g) * mul
        return t.to(BF16).requires_grad_(True)

    x = leaf(M, H)
    w1, b1, w2 = leaf(F, H, mul=0.1), leaf(F, mul=0.2), leaf(H, F, mul=0.05)
    dout = torch.randn(M, H, device="cuda", generator=g).to(BF16)
    leaves = {"x": x, "w1": w1, "b1": b1, "w2": w2}
    fc1_seed = _Anchor()

    def finish(mod, pre, out):
        grads = torch.autograd.grad(out, list(leaves.values()), dout)
        r = {"out": out.detach(), "pre": pre.detach()}
        r.update({"d" + k: v for k, v in zip(leaves, grads)})
        r.update(_state_of(mod))
        return r

    def unfused(mod, fc1=None):
        fc1 = fc1 or _clone_anchor(fc1_seed)
        pre = fp8_linear(x, w1, module=fc1)
        y = ops.bias_gelu(pre, b1)
        return finish(mod, pre, fp8_linear(y, w2, module=mod))

    calls = []
    real = ops.bias_gelu_fp8
    monkeypatch.setattr(ops, "bias_gelu_fp8",
                        lambda *a: calls.append(1) or real(*a))

    def fused(mod):
        pre = fp8_linear(x, w1, module=_clone_anchor(fc1_seed))
        return finish(mod, pre, fp8_gelu_linear(pre, b1, w2, mod))

    seed = _Anchor()
    unfused(seed, fc1_seed)
    _compare_runs(unfused, fused, seed)
    assert len(calls) == 1, "the fused kernel was not on the path"


# --------------------------------------------------------------- model level

STEPS = 3


def _tiny_gpt():
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    cfg = GPTConfig(hidden_size=256, num_layers=2, num_heads=4, seq_len=128,
                    vocab_size=1024)
    return GPTModel(cfg, None, 1, BF16, torch.device("cuda"), init_seed=1)


def _ids():
    return torch.randint(0, 1024, (4, 128), generator=torch.Generator()
                         .manual_seed(5)).cuda()


class _Spy:
    def __init__(self, monkeypatch):
        from alpa_amd import ops
        self.ln = self.gelu = 0
        real_ln, real_gelu = ops.add_layer_norm_fp8, ops.bias_gelu_fp8

        def ln(*a):
            self.ln += 1
            return real_ln(*a)

        def gelu(*a):
            self.gelu += 1
            return real_gelu(*a)

        monkeypatch.setattr(ops, "add_layer_norm_fp8", ln)
        monkeypatch.setattr(ops, "bias_gelu_fp8", gelu)


def _train(fused, wgrad=True, steps=STEPS):
    """Losses of `steps` AdamW steps of the 2-layer GPT under fp8 GEMMs."""
    from alpa_amd.global_env import global_config
    from alpa_amd.ops import fp8 as f8
    old = (global_config.fp8_gemm, global_config.fp8_fused_quant,
           global_config.fp8_wgrad)
    global_config.fp8_gemm = True
    global_config.fp8_fused_quant = fused
    global_config.fp8_wgrad = wgrad
    try:
        m = _tiny_gpt()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        ids = _ids()
        losses = []
        for _ in range(steps):
            loss = m.loss(ids, ids)
            opt.zero_grad()
            loss.backward()
            opt.step()
            f8.bump_epoch()
            losses.append(loss.detach())
        return torch.stack(losses).double().cpu()
    finally:
        (global_config.fp8_gemm, global_config.fp8_fused_quant,
         global_config.fp8_wgrad) = old


def test_gpt_losses_unchanged_by_the_flag(monkeypatch):
    spy = _Spy(monkeypatch)
    off1 = _train(False)
    off2 = _train(False)
    assert spy.ln == 0 and spy.gelu == 0, "flag off must not reach the ops"
    on = _train(True)
    # 2 layers x (ln1->qkv, ln2->fc1) and 2 x fc2, on every step after the
    # first (which seeds the delayed scales through the unfused path)
    assert spy.ln == 4 * (STEPS - 1) and spy.gelu == 2 * (STEPS - 1), \
        (spy.ln, spy.gelu)
    tol = (off1 - off2).abs().max().item()
    diff = (on - off1).abs().max().item()
    print(f"losses off {off1.tolist()} on {on.tolist()}; on-vs-off {diff:.3g},"
          f" off run-to-run {tol:.3g}")
    assert torch.isfinite(on).all()
    assert diff <= tol, (diff, tol)


def test_flag_without_fp8_wgrad_stays_unfused(monkeypatch):
    spy = _Spy(monkeypatch)
    losses = _train(True, wgrad=False, steps=2)
    assert spy.ln == 0 and spy.gelu == 0
    assert torch.isfinite(losses).all()


def test_fused_route_in_a_captured_graph(monkeypatch):
    """Eager warm-up (seeds the scales, then runs the fused kernels once),
    capture of the whole step, replays: finite and decreasing loss."""
    import alpa_amd as aa
    from alpa_amd.global_env import global_config
    from alpa_amd.models.gpt import GPTConfig, GPTModel
    spy = _Spy(monkeypatch)
    old = (global_config.fp8_gemm, global_config.fp8_fused_quant,
           global_config.fp8_wgrad)
    global_config.fp8_gemm = True
    global_config.fp8_fused_quant = True
    global_config.fp8_wgrad = True
    try:
        aa.init()
        cfg = GPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                        seq_len=128, vocab_size=1024)
        method = aa.ShardParallel(logical_mesh_shape=(1, 1))

        def build(mesh=None, axis=1, dtype=BF16, device=None):
            return GPTModel(cfg, mesh, axis, dtype, device, init_seed=1)

        state = aa.TrainState.create(build, method, lr=1e-3)
        step = aa.parallelize(lambda m, b: m.loss(b[0], b[1]),
                              method=method)
        batch = (_ids(), _ids())
        first = float(step(state, batch))
        step(state, batch)
        assert spy.ln == 4 and spy.gelu == 2
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = step(state, batch)
        assert spy.ln == 8 and spy.gelu == 4, "capture left the fused route"
        losses = [first]
        for _ in range(4):
            graph.replay()
            losses.append(float(loss))
        assert all(l == l and abs(l) != float("inf") for l in losses), losses
        assert losses[-1] < losses[1] < losses[0], losses
    finally:
        (global_config.fp8_gemm, global_config.fp8_fused_quant,
         global_config.fp8_wgrad) = old
