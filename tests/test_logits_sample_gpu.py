"""ops.logits_topk and ops.sample_logits (csrc/logits_sample.hip) against
reference.logits_topk / reference.sample_logits on CPU copies, and the paths
that use them: the captured sampling loop and beam search."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alpa_amd import ops
from alpa_amd.global_env import global_config
from alpa_amd.ops import reference as ref

DTYPES = [torch.bfloat16, torch.float32]
INV_T = [1.0, 0.6, 1.7]
WIDTHS = {"k": lambda seg, k: k, "520": lambda seg, k: 520,
          "seg": lambda seg, k: seg, "seg+8": lambda seg, k: seg + 8,
          "2seg+24": lambda seg, k: 2 * seg + 24,
          "50272": lambda seg, k: 50272}


def _rows(V, dtype, seed=0):
    """[3, V] randn logits as a row-strided view of a wider buffer."""
    gen = torch.Generator().manual_seed(seed + V)
    buf = torch.randn(3, (V + 47) // 8 * 8, generator=gen).to(dtype).cuda()
    return buf[:, :V]


def _check(x, k, inv_t, vocab_start=0):
    """vals, idx and m exactly, s to rtol 2e-5: its terms are positive and
    its longest serial fp32 chain is 32 adds in a thread, 12 in the block
    reduction and one per segment (13 at V = 50272 in fp32), 57 <= 64 adds
    of 2^-24 each, plus __expf's few ulp."""
    got = ops.logits_topk(x, k, inv_t, vocab_start)
    want = ref.logits_topk(x.cpu(), k, inv_t.cpu(), vocab_start)
    for g, w, name in zip(got[:3], want[:3], ("vals", "idx", "m")):
        assert torch.equal(g.cpu(), w), name
    s, ws = got[3].cpu().double(), want[3].double()
    print("max rel err of s", float(((s - ws).abs() / ws).max()))
    torch.testing.assert_close(s, ws, rtol=2e-5, atol=0)
    return got


@pytest.mark.parametrize("width", list(WIDTHS))
@pytest.mark.parametrize("k", [1, 5, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_topk_matches_reference(dtype, k, width):
    V = WIDTHS[width](ops.LOGITS_TOPK_SEG[dtype], k)
    x = _rows(V, dtype)
    assert not x.is_contiguous() and ops.logits_topk_ok(x, k)
    _check(x, k, torch.tensor(INV_T).cuda(), vocab_start=3 * V)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_equal_maxima_across_a_segment_boundary(dtype, k):
    seg = ops.LOGITS_TOPK_SEG[dtype]
    x = _rows(2 * seg + 24, dtype)
    x[:, seg - 20:seg + 20] = 9.0
    got = _check(x, k, torch.tensor(INV_T).cuda())
    first = min(k, 40)
    assert got[1][0, :first].tolist() == list(range(seg - 20,
                                                    seg - 20 + first))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_column_shards_compose(dtype):
    """The tp > 1 path on one GPU: the candidates of two column shards,
    merged on the host by (value descending, global column ascending), are
    the whole row's."""
    seg, k = ops.LOGITS_TOPK_SEG[dtype], 64
    x = _rows(2 * seg + 24, dtype)
    inv_t = torch.tensor(INV_T).cuda()
    whole = ops.logits_topk(x, k, inv_t)
    cut = seg + 8
    lo = ops.logits_topk(x[:, :cut], k, inv_t, 0)
    hi = ops.logits_topk(x[:, cut:], k, inv_t, cut)
    vals = torch.cat([lo[0], hi[0]], dim=1).cpu()
    idx = torch.cat([lo[1], hi[1]], dim=1).cpu()
    # shard order is column order, so a stable sort keeps the tie rule
    order = torch.sort(vals, dim=1, descending=True, stable=True).indices
    assert torch.equal(vals.gather(1, order)[:, :k], whole[0].cpu())
    assert torch.equal(idx.gather(1, order)[:, :k], whole[1].cpu())
    assert torch.equal(torch.maximum(lo[2], hi[2]), whole[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_minus_inf_and_nan_rows(dtype):
    V, k = 520, 5
    x = _rows(V, dtype)
    x[0] = -float("inf")
    x[0, 7], x[0, 300] = 0.5, 1.25
    x[1] = -float("inf")
    inv_t = torch.tensor(INV_T).cuda()
    vals, idx, m, s = _check(x[:2], k, inv_t[:2], vocab_start=1000)
    assert idx[0, :2].tolist() == [1300, 1007]
    assert m[1] == -float("inf") and s[1] == 0
    x[2, 77] = float("nan")
    vals, idx, m, s = ops.logits_topk(x, k, inv_t, vocab_start=1000)
    assert torch.isnan(m[2]) and torch.isnan(s[2])
    assert bool(((idx >= 1000) & (idx < 1000 + V)).all())
    tok = ops.sample_logits(x, torch.full((3,), 0.5).cuda(), inv_t, 0, 0.9,
                            k=k)
    assert tok[1] == 0 and 0 <= int(tok[2]) < V
    assert torch.equal(tok[:2].cpu(), ref.sample_logits(
        x[:2].cpu(), torch.full((2,), 0.5), inv_t[:2].cpu(),
        torch.zeros(2).int(), torch.full((2,), 0.9), k=k))


@pytest.mark.parametrize("target", ["first", "middle", "last"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_draw_hits_the_target_candidate(dtype, target):
    """u is the midpoint of the target's interval in the reference's fp64
    CDF; the inputs keep every decision far from fp32 rounding."""
    V, k = 520, 64
    gen = torch.Generator().manual_seed(3)
    perm = torch.stack([torch.randperm(V, generator=gen) for _ in range(3)])
    spaced = -0.37 * torch.arange(V) + 1e-3 * torch.randn(3, V, generator=gen)
    x = torch.empty(3, V).scatter_(1, perm, spaced).to(dtype)
    inv_t = torch.tensor([1.0, 0.7, 1.5])
    top_k = torch.tensor([6, 8, 0], dtype=torch.int32)
    top_p = torch.tensor([1.0, 0.9, 0.6])

    y = ref.logits_topk(x, k, inv_t)[0].double()
    n = torch.where(top_k > 0, top_k, k).long()[:, None]
    j = torch.arange(k)[None]
    p = torch.where(j < n, (y - y[:, :1]).exp(), 0.0)
    e, T = p.cumsum(1) - p, p.sum(1, keepdim=True)
    in_n = (j < n) & (j > 0)
    assert ((e / T - top_p[:, None].double()).abs()[in_n] > 1e-4).all()
    keep = (j < n) & ((j == 0) | (e < top_p[:, None].double() * T))
    kept = keep.sum(1)
    assert kept.tolist() == [6, 6, 2]
    kept_sum = (p * keep).sum(1)
    t = {"first": torch.zeros(3).long(), "middle": kept // 2,
         "last": kept - 1}[target][:, None]
    assert ((p.gather(1, t)[:, 0] / kept_sum) > 1e-3).all()
    u = ((e.gather(1, t) + p.gather(1, t) / 2)[:, 0] / kept_sum).float()

    xg, args = x.cuda(), (inv_t.cuda(), top_k.cuda(), top_p.cuda())
    want = ref.sample_logits(x, u, inv_t, top_k, top_p, k=k)
    assert torch.equal(want, ref.logits_topk(x, k)[1].gather(1, t)[:, 0])
    assert torch.equal(ops.sample_logits(xg, u.cuda(), *args, k=k).cpu(),
                       want)
    if target != "last":
        return
    # the ends of the CDF and the degenerate settings
    top = ref.logits_topk(x, k)[1]
    one = torch.nextafter(torch.ones(3), torch.zeros(3)).cuda()
    assert torch.equal(ops.sample_logits(xg, one, *args, k=k).cpu(),
                       top.gather(1, t)[:, 0])
    zero = torch.zeros(3).cuda()
    assert torch.equal(ops.sample_logits(xg, zero, *args, k=k).cpu(),
                       top[:, 0])
    assert torch.equal(ops.sample_logits(xg, one, args[0], 1, args[2],
                                         k=k).cpu(), top[:, 0])
    assert torch.equal(ops.sample_logits(xg, one, args[0], args[1], 1e-9,
                                         k=k).cpu(), top[:, 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_a_row_does_not_depend_on_its_neighbours(dtype):
    x = _rows(50272, dtype)
    args = (torch.tensor(INV_T).cuda(), torch.tensor([0, 20, 3]).int().cuda(),
            torch.tensor([1.0, 0.8, 0.5]).cuda())
    u = torch.tensor([0.1, 0.7, 0.9]).cuda()
    full = ops.logits_topk(x, 64, args[0], 5) + (
        ops.sample_logits(x, u, *args, k=64),)
    alone = ops.logits_topk(x[1:2], 64, args[0][1:2], 5) + (
        ops.sample_logits(x[1:2], u[1:2], *(a[1:2] for a in args), k=64),)
    for f, a in zip(full, alone):
        assert torch.equal(f[1:2], a)


@pytest.fixture(scope="module")
def tiny_opt():
    import alpa_amd as aa
    from alpa_amd.models.opt import OPTConfig, OPTModel
    aa.init()
    cfg = OPTConfig(hidden_size=256, num_layers=2, num_heads=4,
                    vocab_size=512, max_seq_len=128)
    return OPTModel(cfg, None, 1, torch.bfloat16, "cuda", init_seed=4)


def test_captured_sampling_loop_equals_eager(tiny_opt):
    ids = torch.randint(0, 512, (2, 9),
                        generator=torch.Generator().manual_seed(1)).cuda()
    g1, g2 = (torch.Generator(device="cuda").manual_seed(11)
              for _ in range(2))
    kw = dict(do_sample=True, temperature=0.9, top_k=8, top_p=0.9)
    eager = tiny_opt.generate(ids, max_new_tokens=6, generator=g2, **kw)
    assert torch.equal(
        tiny_opt.generate_graphed(ids, 6, generator=g1, **kw), eager)
    assert not torch.equal(eager, tiny_opt.generate(ids, max_new_tokens=6))


def test_beam_search_scores_with_and_without_the_kernels(tiny_opt,
                                                         monkeypatch):
    ids = torch.randint(0, 512, (2, 9),
                        generator=torch.Generator().manual_seed(2)).cuda()
    logits = tiny_opt.forward_step(ids, tiny_opt.new_cache(2))
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setattr(global_config, "fused_sampling", switch)
        out[switch] = (tiny_opt._log_probs_topk(logits, 4)[0],
                       tiny_opt.beam_search(ids, max_new_tokens=5,
                                            num_beams=3))
    torch.testing.assert_close(out["1"][0], out["0"][0], rtol=0, atol=1e-4)
    assert out["1"][1].shape == out["0"][1].shape == (2, 14)
