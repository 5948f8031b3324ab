"""Head log-probs without logits (ops.functional.head_logprobs), CPU side:
the fp64 reference against log_softmax, the vocab-slice combine, ignored
rows, the kernel gate, and the REALHF_AMD_FUSED_HEAD_LOGPROB wiring of the
PPO and DPO inference calls on the route that CPU takes."""
import pytest
import torch

from realhf_amd.ops import functional as F
from tests.test_fused_logprob import assert_logp_close, hand_combine
from tests.test_interfaces import init_inf, make_model, sft_batch

FLAG = "REALHF_AMD_FUSED_HEAD_LOGPROB"
WARPS = [{}, {"softcap": 2.0}, {"inv_temperature": 1 / 0.7},
         {"softcap": 3.0, "inv_temperature": 2.0}]


def _case(n=6, H=16, V=50, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, H, generator=g, dtype=torch.float64)
    w = torch.randn(V, H, generator=g, dtype=torch.float64) * 4 / H ** 0.5
    labels = torch.randint(0, V, (n,), generator=g)
    labels[0], labels[1], labels[2] = 0, V - 1, -100
    return h, w, labels


def _log_softmax(h, w, labels, softcap=None, inv_temperature=1.0):
    x = h @ w.t()
    x = torch.tanh(x / softcap) * softcap if softcap else x
    lp = torch.log_softmax(x * inv_temperature, -1)
    return lp.gather(1, labels.clamp(min=0).unsqueeze(1)).squeeze(1)


@pytest.mark.parametrize("warp", WARPS)
def test_ref_matches_log_softmax(warp):
    h, w, labels = _case()
    want = _log_softmax(h, w, labels, **warp)
    stats = F.head_logprobs_ref(h, w, labels, **warp)
    assert all(s.dtype == torch.float64 for s in stats)
    assert [float(s[2]) for s in stats] == [0.0, 0.0, 1.0]  # the ignored row
    logp, _ = F.combine_vocab_stats(*stats)
    keep = labels != -100
    torch.testing.assert_close(logp[keep], want[keep], atol=1e-12, rtol=1e-12)
    # the public op: same numbers in fp32, 0 on the ignored row
    got = F.head_logprobs(h.float(), w.float(), labels, **warp)
    assert got.dtype == torch.float32 and got[2] == 0
    assert_logp_close(got[keep], want[keep].float())
    if warp:  # an ignored argument would not pass
        plain = _log_softmax(h, w, labels)
        with pytest.raises(AssertionError):
            assert_logp_close(plain[keep].float(), want[keep].float())


def test_two_slices_combine():
    h, w, labels = _case(V=50)
    kw = {"softcap": 2.0, "inv_temperature": 1 / 0.7}
    parts = [F.head_logprobs_ref(h, w[:20], labels, vocab_start=0, **kw),
             F.head_logprobs_ref(h, w[20:], labels, vocab_start=20, **kw)]
    assert parts[1][0][0] == 0 and parts[0][0][1] == 0  # label in the other slice
    logp, _ = hand_combine(parts)
    full, _ = F.combine_vocab_stats(*F.head_logprobs_ref(h, w, labels, **kw))
    keep = labels != -100  # an ignored row is (0, 0, 1) in every slice
    torch.testing.assert_close(logp[keep], full[keep], atol=1e-12, rtol=1e-12)


def test_supported_gate():
    h = torch.zeros(4, 16, dtype=torch.bfloat16)
    w = torch.zeros(8, 16, dtype=torch.bfloat16)
    gpu = torch.cuda.is_available()
    with torch.no_grad():
        assert not F.head_logprob_supported(h, w)  # CPU
        if gpu:
            h, w = h.cuda(), w.cuda()
        assert F.head_logprob_supported(h, w) == gpu
        assert not F.head_logprob_supported(h.half(), w.half())
        assert not F.head_logprob_supported(h[:, :12], w[:, :12])  # H % 8
        with torch.enable_grad():
            assert not F.head_logprob_supported(h, w)


def _iface(name, temperature):
    from realhf_amd.api.config import Abstraction
    from realhf_amd.api.model import GenerationHyperparameters, make_interface

    args = {}
    if name == "ppo_actor":
        args["gconfig"] = GenerationHyperparameters(
            temperature=temperature).__dict__
    return make_interface(Abstraction(name, args))


@pytest.mark.parametrize("name,key", [("ppo_actor", "packed_ref_logprobs"),
                                      ("dpo", "seqlogp")])
def test_inference_flag_on_matches_off(name, key, monkeypatch):
    model = init_inf(make_model("llama", seed=1))
    batch = sft_batch(model.module.module.config.vocab_size, bs=4)
    if name == "dpo":  # [pos, neg] pairs: two sequences per sample
        lens = [l for x in batch.seqlens["packed_input_ids"] for l in x]
        batch.seqlens = {k: [lens[0:2], lens[2:4]] for k in batch.keys}
        batch.ids = ["a", "b"]
    iface = _iface(name, 0.7)
    monkeypatch.delenv(FLAG, raising=False)
    off = iface.inference(model, batch).data[key]
    calls = []
    real = F.head_logprobs
    monkeypatch.setattr(F, "head_logprobs",
                        lambda *a, **k: calls.append(k) or real(*a, **k))
    assert iface.inference(model, batch).data[key].equal(off) and not calls
    monkeypatch.setenv(FLAG, "1")
    on = iface.inference(model, batch).data[key]
    assert len(calls) == 1
    assert calls[0]["inv_temperature"] == pytest.approx(
        1 / 0.7 if name == "ppo_actor" else 1.0)
    torch.testing.assert_close(on, off, atol=1e-5, rtol=0)


def test_logits_mask_keeps_logits_path(monkeypatch):
    model = init_inf(make_model("llama", seed=1))
    vocab = model.module.module.config.vocab_size
    batch = sft_batch(vocab, bs=2)
    lens = [x[0] for x in batch.seqlens["packed_input_ids"]]
    batch.keys = tuple(batch.keys) + ("packed_logits_mask",)
    batch.seqlens["packed_logits_mask"] = [[l - 1] for l in lens]
    batch.data["packed_logits_mask"] = torch.zeros(
        sum(lens) - 2, vocab, dtype=torch.bool)
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.setattr(F, "head_logprobs", None)  # would raise if called
    out = _iface("ppo_actor", 0.7).inference(model, batch)
    assert out.data["packed_ref_logprobs"].shape == (sum(lens) - 2,)
