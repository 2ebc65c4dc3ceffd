"""reference.logits_topk against log_softmax plus a stable sort, and
per-request sampling in ContinuousBatcher (ops.sample_logits on the CPU)."""
import pytest
import torch

from alpa_amd.models.opt import OPTConfig, OPTModel
from alpa_amd.ops import reference as ref
from alpa_amd.serve.batching import ContinuousBatcher, GenRequest


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_topk_is_log_softmax_and_stable_sort(dtype):
    torch.manual_seed(0)
    x = torch.randn(3, 700).to(dtype)
    x[1, 100:140] = x[1].max()          # a run of equal maxima
    x[2, ::3] = -float("inf")
    inv_t = torch.tensor([1.0, 0.7, 2.5])
    vals, idx, m, s = ref.logits_topk(x, 50, inv_t, vocab_start=1000)
    y = x.float() * inv_t[:, None]
    order = torch.sort(y.double(), dim=-1, descending=True, stable=True)
    assert torch.equal(idx, order.indices[:, :50] + 1000)
    assert torch.equal(vals.double(), order.values[:, :50])
    torch.testing.assert_close(
        vals.double() - m.double()[:, None] - s.double().log()[:, None],
        torch.log_softmax(y.double(), dim=-1).gather(1, idx - 1000),
        rtol=0, atol=1e-6)
    # ties by lower column: the equal maxima come out in column order
    assert idx[1, :40].tolist() == list(range(1100, 1140))


def test_batcher_mixes_sampling_and_greedy_requests():
    cfg = OPTConfig(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
                    max_seq_len=64)
    model = OPTModel(cfg, None, 1, torch.float32, None, init_seed=13)

    def run(requests):
        cb = ContinuousBatcher(model, max_batch=2,
                               generator=torch.Generator().manual_seed(7))
        for r in requests:
            cb.submit(r)
        cb.run_all()

    prompts = [torch.arange(3, 9), torch.arange(20, 25)]
    greedy = [GenRequest(p, 6) for p in prompts]
    run(greedy)
    mixed = [GenRequest(prompts[0], 6),
             GenRequest(prompts[1], 6, do_sample=True, temperature=0.8,
                        top_k=5, top_p=0.95)]
    run(mixed)
    assert mixed[0].output == greedy[0].output
    assert len(mixed[1].output) == 6
    # every sampled token is among the 5 likeliest given what precedes it
    for i, tok in enumerate(mixed[1].output):
        seq = torch.cat([prompts[1], torch.tensor(mixed[1].output[:i],
                                                  dtype=torch.long)])
        logits = model.forward_step(seq[None], model.new_cache(1))
        assert tok in logits[0].topk(5).indices.tolist()
    assert mixed[1].output != greedy[1].output
