"""Shared by test_moe_route_cpu.py and test_moe_route_gpu.py."""
import torch


def tie_free_logits(N, E, seed, shift=4.0, dtype=torch.float32):
    """[N, E]: each row a random permutation of {k/8 : k < E} minus
    `shift`.  Every value is (k - 8*shift)/8 with |k - 8*shift| < 128, so
    it is exact in bf16, and no two entries of a row are equal."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(N, E, generator=g).argsort(dim=-1)
    return (perm.to(torch.float32) / 8.0 - shift).to(dtype)


def assert_top3_distinct(logits):
    """The precondition under which topk-based code has a defined answer."""
    k = min(3, logits.shape[-1])
    top = logits.float().topk(k, dim=-1).values
    assert bool((top[:, :-1] > top[:, 1:]).all()), "top-3 of a row tie"


def check_invariants(r, N, E, C):
    """Structural invariants of a routing result, whatever the logits held.

    - indices in range and distinct, slots in range or -1
    - slot_k[t] >= 0  =>  src[slot_k[t]] == t and slot_k[t] // C == idx_k[t]
    - every src[s] >= 0 is referenced by exactly one (t, k)
    - the occupied slots of each expert are a prefix 0..m-1 of its C slots
    """
    idx = [r.idx1.cpu().long(), r.idx2.cpu().long()]
    slot = [r.slot1.cpu().long(), r.slot2.cpu().long()]
    src = r.src.cpu().long()
    assert src.shape == (E * C,)
    assert bool((idx[0] != idx[1]).all())
    refs = torch.zeros(E * C, dtype=torch.long)
    t = torch.arange(N)
    for i, s in zip(idx, slot):
        assert i.shape == (N,) and s.shape == (N,)
        assert bool(((i >= 0) & (i < E)).all())
        assert bool(((s >= -1) & (s < E * C)).all())
        kept = s >= 0
        assert torch.equal(src[s[kept]], t[kept])
        assert torch.equal(s[kept] // C, i[kept])
        refs.index_add_(0, s[kept], torch.ones_like(s[kept]))
    assert bool(((src >= -1) & (src < N)).all())
    assert torch.equal(refs, (src >= 0).long())
    occ = (src >= 0).view(E, C)
    m = occ.sum(-1, keepdim=True)
    assert torch.equal(occ, torch.arange(C).expand(E, C) < m)
