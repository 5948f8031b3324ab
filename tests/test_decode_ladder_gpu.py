"""The lower rungs of the decode projection ladder at model level: a llama
whose gate/up (N = 96, no multiple of 64) and down (K = 48, no multiple of 32)
projections no skinny kernel takes, so they fall through to the dense GEMM
while QKV and wo keep the slab route; with FP8 weights only QKV and wo have
pairs.  Entry-point call counts, and the fused decode block against eager
decode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

L = 2
STEPS = 4  # decode steps after the prefill
LENS = [9, 5, 7]  # 21 prompt tokens: the prefill's output head is not skinny
NAMES = ("skinny_gemm", "skinny_gemm_nc", "skinny_gemm_fp8",
         "skinny_gemm_fp8_nc", "quantize_rows_e4m3_")


def _llama(seed=7):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=L, hidden_dim=64, n_heads=1, n_kv_heads=1, head_dim=64,
        vocab_size=128, intermediate_dim=48,
    )
    cfg.family = "llama"
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init(std=0.05)
    return m


def _generate(monkeypatch, m, quant, forced=None):
    """A fresh eager-decode session; forced [bs, STEPS + 1]: sample these
    tokens instead (teacher forcing keeps two runs on one token path)."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models import generation as genmod

    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 128, (sum(LENS),), generator=g).cuda()
    cu = torch.tensor([0, 9, 14, 21], dtype=torch.int32, device="cuda")
    gconfig = GenerationHyperparameters(
        max_new_tokens=STEPS + 1, greedy=True, use_hip_graph=False,
        weight_quant=quant)
    real = genmod._sample_from_logits
    step = [0]

    def sample(logits, *a, **kw):
        tokens, logp, mask = real(logits, *a, **kw)
        if forced is not None:
            tokens = forced[:, step[0]]
            logp = torch.log_softmax(logits, -1).gather(
                -1, tokens.unsqueeze(-1)).squeeze(-1)
        step[0] += 1
        return tokens, logp, mask

    m._gen_session = None
    with monkeypatch.context() as mp:
        mp.setattr(genmod, "_sample_from_logits", sample)
        return genmod.generate(m, toks, cu, gconfig)


def test_lower_rungs_dispatch_and_match_eager(monkeypatch):
    monkeypatch.delenv("REALHF_AMD_GEN_WEIGHT_QUANT", raising=False)
    monkeypatch.delenv("REALHF_AMD_NO_FUSED_DECODE", raising=False)
    m = _llama()
    seen = {n: [] for n in NAMES}

    def spy(name):
        real = getattr(C, name)

        def f(*a):
            seen[name].append(a)
            return real(*a)

        monkeypatch.setattr(C, name, f)

    for n in NAMES:
        spy(n)

    def weight_shapes(name):
        return sorted({tuple(a[1].shape) for a in seen[name]})

    # bf16: QKV and wo hand slabs on; gate/up and down reach no skinny entry
    # point; the output head is the only combined call
    out = _generate(monkeypatch, m, None)
    assert out.gen_tokens.shape == (3, STEPS + 1)
    assert len(seen["skinny_gemm_nc"]) == 2 * L * STEPS
    assert weight_shapes("skinny_gemm_nc") == [(64, 64), (192, 64)]
    assert len(seen["skinny_gemm"]) == STEPS
    assert weight_shapes("skinny_gemm") == [(128, 64)]
    for n in NAMES[2:]:
        assert not seen[n], n

    # fp8: only QKV and wo have pairs, and the fp8 entry points see exactly
    # those two
    for v in seen.values():
        v.clear()
    _generate(monkeypatch, m, "fp8_e4m3")
    assert [sorted(d) for d in m._gen_session[1].fp8.pairs] == [["qkv", "wo"]] * L
    assert len(seen["quantize_rows_e4m3_"]) == 2 * L
    assert len(seen["skinny_gemm_fp8_nc"]) == 2 * L * STEPS
    assert weight_shapes("skinny_gemm_fp8_nc") == [(64, 64), (192, 64)]
    assert not seen["skinny_gemm_fp8"]
    assert not seen["skinny_gemm_nc"]
    assert len(seen["skinny_gemm"]) == STEPS

    # eager decode on the same token path: no slab call at all, and the
    # log-probs at the bound test_gemma_model_matches_torch_path uses for a
    # kernel-path model against the torch path
    for v in seen.values():
        v.clear()
    monkeypatch.setenv("REALHF_AMD_NO_FUSED_DECODE", "1")
    ref = _generate(monkeypatch, m, None, forced=out.gen_tokens)
    assert not seen["skinny_gemm_nc"]
    assert len(seen["skinny_gemm"]) == STEPS
    assert torch.equal(ref.gen_tokens, out.gen_tokens)
    print("fused vs eager decode: max |diff| of gen_logprobs",
          (out.gen_logprobs - ref.gen_logprobs).abs().max().item(),
          "max |logprob|", ref.gen_logprobs.abs().max().item())
    torch.testing.assert_close(out.gen_logprobs, ref.gen_logprobs,
                               atol=3e-2, rtol=3e-2)
