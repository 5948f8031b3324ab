"""Gemma-2 on the CPU: the family against transformers' Gemma2ForCausalLM
(eager attention) with every new piece binding, the HF round trips, prefill +
decode against the packed forward, and the flat layout of the other
families."""
import dataclasses

import numpy as np
import pytest
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.api.model import GenerationHyperparameters
from realhf_amd.models import param_layout as PL
from realhf_amd.models.generation import generate
from realhf_amd.models.real_model import ReaLModel

ATOL, RTOL = 2e-4, 2e-3  # test_model_cpu's
LENS = [5, 20, 33]


def _cfg():
    """4 layers (sliding, full, sliding, full); window 8 binds on the 20 and
    33 token sequences; both caps bind; query_pre_attn_scalar != head_dim."""
    fam = hf_reg.get_family("gemma2")
    cfg = fam.make_test_config(
        n_layers=4, hidden_dim=64, n_heads=4, n_kv_heads=2, head_dim=16,
        vocab_size=64, sliding_window=8, attn_logit_softcap=2.0,
        final_logit_softcap=3.0, query_pre_attn_scalar=24.0)
    cfg.dtype = "float32"
    return fam, cfg


def _hf_model(fam, cfg, **override):
    import transformers

    d = dict(fam.config_to_hf(cfg))
    d.update(override)
    hf_cfg = transformers.AutoConfig.for_model(d.pop("model_type"), **d)
    torch.manual_seed(42)
    m = transformers.AutoModelForCausalLM.from_config(
        hf_cfg, attn_implementation="eager").eval().float()
    assert m.config._attn_implementation == "eager"
    # transformers initialises the norm weights to zero, and 1 + 0 would hide
    # a swapped norm mapping; larger projections make the caps bind
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif p.ndim == 2:
                p.mul_(4.0)
    return m


def _ids(vocab):
    # token 0 is transformers' padding_idx: keep it out of the batch
    rng = np.random.RandomState(0)
    ids = [torch.from_numpy(rng.randint(1, vocab, size=l)).long() for l in LENS]
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32)
    return ids, torch.cat(ids), cu


def _hf_logp(m, ids):
    with torch.no_grad():
        return torch.cat([
            torch.log_softmax(m(input_ids=x.unsqueeze(0)).logits[0].float(), -1)
            for x in ids])


def _our_logp(model, packed, cu):
    with torch.no_grad():
        out = model(packed_input_ids=packed, cu_seqlens=cu, max_seqlen=max(LENS))
    return torch.log_softmax(out.float(), -1)


@pytest.fixture(scope="module")
def oracle():
    fam, cfg = _cfg()
    m = _hf_model(fam, cfg)
    ids, packed, cu = _ids(cfg.vocab_size)
    return fam, cfg, m, ids, packed, cu, _hf_logp(m, ids)


def test_gemma2_logits_match_hf(oracle):
    fam, cfg, m, ids, packed, cu, ref = oracle
    assert m.config.layer_types == ["sliding_attention", "full_attention"] * 2
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf_state_dict(model, "gemma2", m.state_dict())
    torch.testing.assert_close(_our_logp(model, packed, cu), ref,
                               atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("override", [
    {"attn_logit_softcapping": None},
    {"final_logit_softcapping": None},
    {"query_pre_attn_scalar": 16},  # = head_dim
    {"sliding_window": 4096},  # never binds
    {"layer_types": ["full_attention", "sliding_attention"] * 2},
], ids=lambda o: next(iter(o)))
def test_oracle_tells_the_pieces_apart(oracle, override):
    """Dropping one piece on the HF side moves its logits by more than the
    tolerance, so the comparison above exercises that piece."""
    fam, cfg, m, ids, packed, cu, ref = oracle
    m2 = _hf_model(fam, cfg, **override)
    m2.load_state_dict(m.state_dict())
    other = _hf_logp(m2, ids)
    assert not torch.allclose(other, ref, atol=10 * ATOL, rtol=10 * RTOL)


@pytest.mark.parametrize("a,b", [
    ("input_layernorm", "post_attention_layernorm"),
    ("post_attention_layernorm", "pre_feedforward_layernorm"),
    ("pre_feedforward_layernorm", "post_feedforward_layernorm"),
])
def test_oracle_tells_the_norms_apart(oracle, a, b):
    """Swapping two of a layer's norm weights moves the HF logits."""
    fam, cfg, m, ids, packed, cu, ref = oracle
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    ka, kb = (f"model.layers.1.{n}.weight" for n in (a, b))
    sd[ka], sd[kb] = sd[kb], sd[ka]
    m2 = _hf_model(fam, cfg)
    m2.load_state_dict(sd)
    assert not torch.allclose(_hf_logp(m2, ids), ref, atol=10 * ATOL,
                              rtol=10 * RTOL)


def test_config_round_trip(oracle):
    fam, cfg, m, *_ = oracle
    back = fam.config_from_hf(fam.config_to_hf(cfg))
    back.dtype = cfg.dtype
    assert dataclasses.asdict(back) == dataclasses.asdict(cfg)
    # and from what transformers itself writes (rope_theta in rope_parameters)
    d = m.config.to_dict()
    d["rope_parameters"] = {"rope_type": "default", "rope_theta": 12345.0}
    d.pop("rope_theta", None)
    got = fam.config_from_hf(d)
    assert got.rotary_base == 12345.0
    assert got.attn_logit_softcap == 2.0 and got.final_logit_softcap == 3.0
    assert got.query_pre_attn_scalar == 24.0 and got.post_norms
    assert got.sliding_window == 8
    assert got.sliding_window_layers == [True, False, True, False]
    assert got.param_count() == cfg.param_count()


def test_param_count_counts_post_norms():
    """param_count() grows by what the layout grows by: two [hidden] norm
    vectors per layer."""
    fam, cfg = _cfg()
    plain = dataclasses.replace(cfg, post_norms=False)
    extra = 2 * cfg.hidden_dim * cfg.n_layers
    assert cfg.param_count() - plain.param_count() == extra

    def numel(c):
        return sum(int(np.prod(PL.key_full_shape(c, k))) for k in PL.all_keys(c))

    assert numel(cfg) - numel(plain) == extra


def test_save_load_through_transformers(oracle, tmp_path):
    import transformers

    fam, cfg, m, ids, packed, cu, ref = oracle
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf_state_dict(model, "gemma2", m.state_dict())
    hf_reg.save_to_hf(model, "gemma2", str(tmp_path))
    m2 = transformers.AutoModelForCausalLM.from_pretrained(
        str(tmp_path), attn_implementation="eager").eval().float()
    assert type(m2).__name__ == "Gemma2ForCausalLM"
    torch.testing.assert_close(_hf_logp(m2, ids), ref, atol=ATOL, rtol=RTOL)
    # and back into a fresh model from the files
    cfg2 = hf_reg.config_from_hf_path("gemma2", str(tmp_path))
    cfg2.dtype = "float32"
    model2 = ReaLModel(cfg2, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf(model2, "gemma2", str(tmp_path))
    torch.testing.assert_close(_our_logp(model2, packed, cu), ref,
                               atol=ATOL, rtol=RTOL)


def test_prefill_decode_matches_packed_forward(oracle):
    """Prefill + 12 greedy decode steps on the CPU routes: the context grows
    from 5 / 7 past the window of 8, so sliding and full layers see different
    key ranges.  Each step's token and log-prob equal the packed forward's."""
    fam, cfg, m, *_ = oracle
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf_state_dict(model, "gemma2", m.state_dict())
    rng = np.random.RandomState(5)
    plens, n_new = [5, 7], 12
    prompts = [torch.from_numpy(rng.randint(1, cfg.vocab_size, size=l)).long()
               for l in plens]
    cu = torch.tensor([0] + list(np.cumsum(plens)), dtype=torch.int32)
    g = GenerationHyperparameters(max_new_tokens=n_new, greedy=True,
                                  use_hip_graph=False)
    out = generate(model, torch.cat(prompts), cu, g, eos_token_id=None,
                   pad_token_id=0)
    for i, p in enumerate(prompts):
        full = torch.cat([p, out.gen_tokens[i]])
        L = full.shape[0]
        with torch.no_grad():
            logits = model(packed_input_ids=full,
                           cu_seqlens=torch.tensor([0, L], dtype=torch.int32),
                           max_seqlen=L)
        lp = torch.log_softmax(logits.float(), -1)[len(p) - 1:L - 1]
        assert lp.argmax(-1).tolist() == out.gen_tokens[i].tolist()
        torch.testing.assert_close(
            lp.gather(-1, out.gen_tokens[i].unsqueeze(-1)).squeeze(-1),
            out.gen_logprobs[i].float(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("family", ["llama", "gemma", "mixtral"])
def test_other_families_have_no_post_ln_keys(family):
    cfg = hf_reg.get_family(family).make_test_config()
    assert not cfg.post_norms
    assert not any("post_ln" in k for k in PL.all_keys(cfg))


def test_gemma2_layout_keys():
    fam, cfg = _cfg()
    ks = PL.tblock_keys(cfg, 1)
    assert ks == [
        "1.attn.ln.weight", "1.attn.wq.weight", "1.attn.wk.weight",
        "1.attn.wv.weight", "1.attn.wo.weight", "1.attn.post_ln.weight",
        "1.mlp.ln.weight", "1.mlp.gate.weight", "1.mlp.up.weight",
        "1.mlp.down.weight", "1.mlp.post_ln.weight"]
    for k in ("1.attn.post_ln.weight", "1.mlp.post_ln.weight"):
        assert PL.key_kind(k) == PL.REPLICATED
        assert PL.key_local_shape(cfg, k, 1, 2) == (cfg.hidden_dim,)
    assert hf_reg.get_family("gemma2").hf_deps(cfg, "2.mlp.ln.weight") == [
        "model.layers.1.pre_feedforward_layernorm.weight"]
    assert hf_reg.get_family("gemma2").hf_deps(cfg, "2.attn.post_ln.weight") == [
        "model.layers.1.post_attention_layernorm.weight"]
