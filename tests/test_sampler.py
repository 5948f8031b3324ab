"""sample_logits_ref (the CPU sampler and the kernel's oracle) against
today's torch sampler, its inverse CDF at the ends of [0, 1), and how
GenerationHyperparameters.sampler resolves and drives generate()."""
import math

import pytest
import torch

from realhf_amd.api.model import GenerationHyperparameters
from realhf_amd.models import generation as gen
from realhf_amd.ops import functional as F

ENV = "REALHF_AMD_GEN_SAMPLER"
BELOW_ONE = math.nextafter(1.0, 0.0)  # fp64; the fp32 one rounds to it


@pytest.mark.parametrize("V,k,p", [(1031, 5, 0.7), (1031, 200, 1.0),
                                   (32000, 1000, 0.9)])
def test_kept_set_matches_torch_sampler(V, k, p):
    torch.manual_seed(V + k)
    # a permuted ramp: randn repeats values at V = 32000
    logits = torch.stack([torch.linspace(-9, 9, V)[torch.randperm(V)]
                          for _ in range(4)])
    assert all(r.unique().numel() == V for r in logits / 0.7)  # no ties
    g = GenerationHyperparameters(top_k=k, top_p=p, temperature=0.7)
    _, _, want = gen._sample_from_logits(
        logits, g, torch.Generator().manual_seed(0), return_mask=True)
    tok, logp, mask = F.sample_logits_ref(logits, torch.rand(4), 0.7, k, p,
                                          False, True)
    assert torch.equal(mask, want) and 0 < (~mask).sum() <= 4 * k
    assert not mask.gather(1, tok[:, None]).any()
    filtered = (logits / 0.7).masked_fill(mask, float("-inf"))
    torch.testing.assert_close(
        logp, torch.log_softmax(filtered, -1).gather(1, tok[:, None])[:, 0])


@pytest.mark.parametrize("k,p", [(5, 0.7), (0, 1.0)], ids=["select", "full"])
def test_inverse_cdf_ends(k, p):
    torch.manual_seed(3)
    x = torch.randn(3, 257, dtype=torch.float64) * 3
    x[:, 7] = float("-inf")
    _, _, mask = F.sample_logits_ref(x, torch.zeros(3), 1.0, k, p, False, True)
    kept = (~mask) * torch.arange(257)
    if k:  # candidate order: the largest first, the smallest kept one last
        first = x.argmax(-1)
        last = x.masked_fill(mask, float("inf")).argmin(-1)
    else:  # index order, and -inf is never returned
        first, last = torch.zeros(3, dtype=torch.long), kept.amax(-1)
        assert mask[:, 7].all() and mask.sum() == 3
    for u, want in ((0.0, first), (BELOW_ONE, last)):
        tok, _, _ = F.sample_logits_ref(
            x, torch.full((3,), u, dtype=torch.float64), 1.0, k, p, False, True)
        assert torch.equal(tok, want)


def test_one_hot_row():
    x = torch.full((2, 300), float("-inf"))
    x[0, 41] = 2.0
    x[1, 299] = -3.0
    for k, p, greedy in ((5, 0.9, False), (0, 1.0, False), (0, 1.0, True)):
        for want_mask in (False, True):
            tok, logp, _ = F.sample_logits_ref(x, torch.tensor([0.3, 0.99]),
                                               0.7, k, p, greedy, want_mask)
            assert tok.tolist() == [41, 299] and logp.tolist() == [0.0, 0.0]


def test_sampler_field_resolution(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    G = GenerationHyperparameters
    assert G().sampler is None and gen.resolve_sampler(G()) == "torch"
    monkeypatch.setenv(ENV, "hip")
    assert gen.resolve_sampler(G()) == "hip"
    assert gen.resolve_sampler(G(sampler="torch")) == "torch"
    monkeypatch.setenv(ENV, "torch")
    assert gen.resolve_sampler(G(sampler="hip")) == "hip"
    with pytest.raises(ValueError):
        gen.resolve_sampler(G(sampler="triton"))
    monkeypatch.setenv(ENV, "fast")
    with pytest.raises(ValueError):
        gen.resolve_sampler(G())


def test_generate_hip_sampler_on_cpu_is_a_function_of_the_seed(monkeypatch):
    from realhf_amd.models.hf import llama
    from realhf_amd.models.real_model import ReaLModel

    monkeypatch.delenv(ENV, raising=False)
    cfg = llama.make_test_config(vocab_size=64)
    m = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    torch.manual_seed(0)
    m.random_init()
    packed = torch.randint(0, 64, (14,), generator=torch.Generator().manual_seed(1))
    cu = torch.tensor([0, 6, 14], dtype=torch.int32)

    def run(seed, **kw):
        g = GenerationHyperparameters(max_new_tokens=6, top_k=8, top_p=0.9,
                                      use_hip_graph=False, sampler="hip", **kw)
        return gen.generate(m, packed, cu, g,
                            generator=torch.Generator().manual_seed(seed))

    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a.gen_tokens, b.gen_tokens)
    assert torch.equal(a.gen_logprobs, b.gen_logprobs)
    assert not torch.equal(a.gen_tokens, c.gen_tokens)
    masked = run(5, force_no_logits_mask=False)
    assert torch.equal(masked.gen_tokens, a.gen_tokens)
    assert masked.logits_mask.shape == (2, 6, 64)
    assert not masked.logits_mask.gather(2, a.gen_tokens[..., None]).any()
