"""Qwen3 on the CPU: the family against transformers' Qwen3ForCausalLM with
random, different q_norm / k_norm weights, the HF round trips, the flat
layout, the reference op's gradients, the untouched decode blockers, and the
q_ln / k_ln gradients under tensor parallelism (partial sums over heads)."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.api.model import GenerationHyperparameters
from realhf_amd.base.testing import LocalMultiProcessTest
from realhf_amd.models import layers
from realhf_amd.models import param_layout as PL
from realhf_amd.models.generation import (generate, kv_quant_blocker,
                                          weight_quant_blocker)
from realhf_amd.models.real_model import ReaLModel
from realhf_amd.ops import functional as ops

ATOL, RTOL = 2e-4, 2e-3  # test_model_cpu's
LENS = [7, 19]


def _cfg():
    """2 layers, hidden 64, 4 heads on 2 kv heads, head_dim 32 != 64 / 4."""
    fam = hf_reg.get_family("qwen3")
    cfg = fam.make_test_config(
        n_layers=2, hidden_dim=64, n_heads=4, n_kv_heads=2, head_dim=32,
        vocab_size=64)
    cfg.dtype = "float32"
    return fam, cfg


def _hf_model(fam, cfg):
    import transformers

    d = dict(fam.config_to_hf(cfg))
    hf_cfg = transformers.AutoConfig.for_model(d.pop("model_type"), **d)
    torch.manual_seed(42)
    m = transformers.AutoModelForCausalLM.from_config(
        hf_cfg, attn_implementation="eager").eval().float()
    assert type(m).__name__ == "Qwen3ForCausalLM"
    # the all-ones norm init would hide a swapped or omitted q/k norm
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.5 * torch.randn(p.shape, generator=g))
            elif p.ndim == 2:
                p.mul_(4.0)
    return m


def _ids(vocab):
    rng = np.random.RandomState(0)
    ids = [torch.from_numpy(rng.randint(1, vocab, size=l)).long() for l in LENS]
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32)
    return ids, torch.cat(ids), cu


def _hf_logits(m, ids):
    with torch.no_grad():
        return torch.cat([m(input_ids=x.unsqueeze(0)).logits[0].float()
                          for x in ids])


def _our_logits(model, packed, cu):
    with torch.no_grad():
        return model(packed_input_ids=packed, cu_seqlens=cu,
                     max_seqlen=max(LENS)).float()


@pytest.fixture(scope="module")
def oracle():
    fam, cfg = _cfg()
    m = _hf_model(fam, cfg)
    ids, packed, cu = _ids(cfg.vocab_size)
    return fam, cfg, m, ids, packed, cu, _hf_logits(m, ids)


def _loaded(cfg, m):
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf_state_dict(model, "qwen3", m.state_dict())
    return model


def test_qwen3_logits_match_hf(oracle):
    fam, cfg, m, ids, packed, cu, ref = oracle
    sd = m.state_dict()
    qn = sd["model.layers.0.self_attn.q_norm.weight"]
    kn = sd["model.layers.0.self_attn.k_norm.weight"]
    assert qn.shape == kn.shape == (cfg.head_dim,) and not torch.equal(qn, kn)
    model = _loaded(cfg, m)
    torch.testing.assert_close(_our_logits(model, packed, cu), ref,
                               atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("how", ["swap", "ones"])
def test_oracle_tells_the_qk_norms_apart(oracle, how):
    """Swapping q_norm and k_norm, or dropping them (all ones), moves the HF
    logits by more than the tolerance."""
    fam, cfg, m, ids, packed, cu, ref = oracle
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    kq, kk = (f"model.layers.1.self_attn.{n}.weight" for n in ("q_norm", "k_norm"))
    if how == "swap":
        sd[kq], sd[kk] = sd[kk], sd[kq]
    else:
        sd[kq], sd[kk] = torch.ones_like(sd[kq]), torch.ones_like(sd[kk])
    m2 = _hf_model(fam, cfg)
    m2.load_state_dict(sd)
    assert not torch.allclose(_hf_logits(m2, ids), ref, atol=10 * ATOL,
                              rtol=10 * RTOL)


def test_generation_through_kv_cache_matches_no_cache_forward(oracle):
    fam, cfg, m, *_ = oracle
    model = _loaded(cfg, m)
    rng = np.random.RandomState(5)
    plens, n_new = [5, 9], 8
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
        assert (logits[len(p) - 1:L - 1].argmax(-1).tolist()
                == out.gen_tokens[i].tolist())
        # and transformers agrees on the greedy tokens
        with torch.no_grad():
            hf = m(input_ids=full.unsqueeze(0)).logits[0]
        assert (hf[len(p) - 1:L - 1].argmax(-1).tolist()
                == out.gen_tokens[i].tolist())


def test_config_round_trip(oracle):
    fam, cfg, m, *_ = oracle
    back = fam.config_from_hf(fam.config_to_hf(cfg))
    back.dtype = cfg.dtype
    assert dataclasses.asdict(back) == dataclasses.asdict(cfg)
    assert back.qk_rmsnorm and not back.qk_layernorm
    # from what transformers 5 itself writes: rope_theta in rope_parameters
    d = m.config.to_dict()
    d["rope_parameters"] = {"rope_type": "default", "rope_theta": 12345.0}
    d.pop("rope_theta", None)
    got = fam.config_from_hf(d)
    assert got.rotary_base == 12345.0
    assert got.head_dim == 32 and got.qk_rmsnorm
    assert not got.use_attention_bias
    assert got.layer_norm_epsilon == cfg.layer_norm_epsilon
    assert got.tied_embedding == cfg.tied_embedding
    assert got.param_count() == cfg.param_count()
    # Qwen3-0.6B's geometry: head_dim is not hidden / heads
    small = fam.config_from_hf(dict(
        num_hidden_layers=28, hidden_size=1024, num_attention_heads=16,
        num_key_value_heads=8, head_dim=128, intermediate_size=3072,
        vocab_size=151936, tie_word_embeddings=True, rms_norm_eps=1e-6,
        rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}))
    assert small.head_dim == 128 and small.tied_embedding
    assert small.rotary_base == 1000000.0
    # linear scaling inside rope_parameters
    scaled = fam.config_from_hf(dict(
        d, rope_parameters={"rope_type": "linear", "factor": 2.0,
                            "rope_theta": 1e6}))
    assert scaled.rotary_scaling == 2.0 and scaled.rotary_scaling_type == "linear"
    with pytest.raises(NotImplementedError):
        fam.config_from_hf(dict(d, rope_scaling={"rope_type": "yarn", "factor": 4.0}))


def test_sliding_window_raises(oracle):
    fam, cfg, m, *_ = oracle
    d = m.config.to_dict()
    d["use_sliding_window"] = True
    with pytest.raises(NotImplementedError):
        fam.config_from_hf(d)


def test_save_load_through_transformers(oracle, tmp_path):
    import transformers

    fam, cfg, m, ids, packed, cu, ref = oracle
    model = _loaded(cfg, m)
    hf_reg.save_to_hf(model, "qwen3", str(tmp_path))
    m2 = transformers.AutoModelForCausalLM.from_pretrained(
        str(tmp_path), attn_implementation="eager").eval().float()
    assert type(m2).__name__ == "Qwen3ForCausalLM"
    torch.testing.assert_close(_hf_logits(m2, ids), ref, atol=ATOL, rtol=RTOL)
    cfg2 = hf_reg.config_from_hf_path("qwen3", str(tmp_path))
    cfg2.dtype = "float32"
    model2 = ReaLModel(cfg2, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf(model2, "qwen3", str(tmp_path))
    torch.testing.assert_close(_our_logits(model2, packed, cu), ref,
                               atol=ATOL, rtol=RTOL)


def test_layout(oracle):
    fam, cfg, m, *_ = oracle
    ks = PL.tblock_keys(cfg, 1)
    assert ks == [
        "1.attn.ln.weight", "1.attn.wq.weight", "1.attn.wk.weight",
        "1.attn.wv.weight", "1.attn.wo.weight", "1.attn.q_ln.weight",
        "1.attn.k_ln.weight", "1.mlp.ln.weight", "1.mlp.gate.weight",
        "1.mlp.up.weight", "1.mlp.down.weight"]
    for k in ("1.attn.q_ln.weight", "1.attn.k_ln.weight"):
        assert PL.key_kind(k) == PL.REPLICATED
        assert PL.key_full_shape(cfg, k) == (cfg.head_dim,)
        assert PL.key_local_shape(cfg, k, 1, 2) == (cfg.head_dim,)
        assert PL.grad_is_head_partial(k)
    assert not PL.grad_is_head_partial("1.attn.ln.weight")
    assert fam.hf_deps(cfg, "2.attn.k_ln.weight") == [
        "model.layers.1.self_attn.k_norm.weight"]
    model = _loaded(cfg, m)
    blk = model.layers[1]
    params = model._params
    merged = layers._maybe_merged(
        params, ["1.attn.wq.weight", "1.attn.wk.weight", "1.attn.wv.weight"],
        (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim)
    assert merged is not None
    assert merged.data_ptr() == params["1.attn.wq.weight"].data_ptr()
    assert "qkv" in blk.decode_weights()
    n_hf = sum(p.numel() for p in m.parameters())
    assert cfg.param_count() == n_hf
    assert sum(int(np.prod(PL.key_full_shape(cfg, k)))
               for k in PL.all_keys(cfg)) == n_hf


@pytest.mark.parametrize("family", ["llama", "qwen2", "gemma2", "mixtral"])
def test_other_families_keep_their_keys(family):
    cfg = hf_reg.get_family(family).make_test_config()
    assert not cfg.qk_rmsnorm
    ks = PL.all_keys(cfg)
    assert not any("q_ln" in k or "k_ln" in k for k in ks)
    on = dataclasses.replace(cfg, qk_rmsnorm=True)
    extra = [k for k in PL.all_keys(on) if k not in ks]
    assert [k for k in PL.all_keys(on) if k in ks] == ks
    assert len(extra) == 2 * cfg.n_layers
    assert on.param_count() - cfg.param_count() == 2 * cfg.head_dim * cfg.n_layers


@pytest.mark.parametrize("rope", [True, False])
def test_reference_gradients_match_unfused_composition(rope):
    torch.manual_seed(3)
    total, nq, nkv, hd = 11, 4, 2, 16
    qkv = torch.randn(total, (nq + 2 * nkv) * hd)
    q_w = (1 + 0.5 * torch.randn(hd)).requires_grad_()
    k_w = (1 + 0.5 * torch.randn(hd)).requires_grad_()
    pos = torch.cat([torch.arange(4), torch.arange(7)])
    cos, sin = ops.rotary_cache.get(hd, 16, 10000.0, "cpu")
    eps = 1e-6

    def split(x):
        q, k, _ = x.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
        return q.reshape(total, nq, hd), k.reshape(total, nkv, hd)

    def unfused(x, w):
        n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
        if not rope:
            return n
        c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
        x1, x2 = n[..., : hd // 2], n[..., hd // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)

    gq = torch.randn(total, nq, hd)
    gk = torch.randn(total, nkv, hd)
    grads = []
    for fused in (True, False):
        x = qkv.clone().requires_grad_()
        q, k = split(x)
        if fused:
            qo, ko = ops.qk_norm_rope(q, k, q_w, k_w, eps,
                                      cos if rope else None,
                                      sin if rope else None, pos)
        else:
            qo, ko = unfused(q, q_w), unfused(k, k_w)
        grads.append(torch.autograd.grad((qo * gq).sum() + (ko * gk).sum(),
                                         [x, q_w, k_w]) + (qo, ko))
    for a, b in zip(*grads):
        # both in fp32; they differ by the order of the operations only
        torch.testing.assert_close(a, b, atol=1e-5, rtol=1e-4)


def _stub(**kw):
    """What the blockers read of a model: qk_layernorm and head_dim only."""
    cfg = types.SimpleNamespace(qk_layernorm=kw.pop("qk_layernorm", False),
                                head_dim=128)
    return types.SimpleNamespace(
        config=cfg, lora_flat=None, dtype=torch.bfloat16, pp_size=1,
        flat_param=types.SimpleNamespace(is_cuda=True))


def test_blockers_unchanged(monkeypatch):
    monkeypatch.delenv("REALHF_AMD_NO_FUSED_DECODE", raising=False)
    # a stub without qk_rmsnorm: the blockers do not read the new field
    for blocker in (weight_quant_blocker, kv_quant_blocker):
        assert "qk_layernorm" in blocker(_stub(qk_layernorm=True))
        assert blocker(_stub()) is None
    assert layers.fused_decode_blocker(
        _stub(qk_layernorm=True).config, torch.bfloat16, True, False) == "qk_layernorm"
    # a qk_rmsnorm model is not blocked
    fam = hf_reg.get_family("qwen3")
    cfg = fam.make_test_config(head_dim=128)
    assert cfg.qk_rmsnorm and not cfg.qk_layernorm
    assert layers.fused_decode_blocker(cfg, torch.bfloat16, True, False) is None
    m = types.SimpleNamespace(
        config=cfg, lora_flat=None, dtype=torch.bfloat16, pp_size=1,
        flat_param=types.SimpleNamespace(is_cuda=True))
    assert weight_quant_blocker(m) is None and kv_quant_blocker(m) is None


# ---------------------------------------------------------------------------
# tensor parallelism: q_ln / k_ln gradients are partial sums over heads
# ---------------------------------------------------------------------------
def _tp_grad_worker(sp):
    import torch.distributed as dist

    from realhf_amd.base import constants
    from realhf_amd.base.testing import init_global_constants
    from realhf_amd.parallel import mappings
    from realhf_amd.parallel.ddp import OptimizerConfig, ZeRO1Optimizer
    from tests.test_realloc import _fill_model_from_full, _full_reference_sd

    cfg = hf_reg.get_family("qwen3").make_test_config(
        n_layers=2, hidden_dim=64, n_heads=8, n_kv_heads=4, head_dim=16,
        vocab_size=128)
    cfg.dtype = "float32"
    sd = _full_reference_sd(cfg, seed=11)
    for k in sd:  # keep the residual stream tame: randn weights everywhere
        if sd[k].ndim == 2:
            sd[k] *= 0.1
    init_global_constants(num_dp=1, num_tp=2, num_pp=1, model_name="m",
                          sequence_parallel=sp)
    g = constants.grid_of("m")
    rng = np.random.RandomState(5)
    lens = [8, 12, 16]  # SP needs total % tp == 0
    packed = torch.from_numpy(rng.randint(0, cfg.vocab_size, size=sum(lens))).long()
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    gout = torch.from_numpy(rng.randn(sum(lens), cfg.vocab_size)).float()

    full = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    _fill_model_from_full(full, cfg, sd)
    for p in full._params.values():
        p.requires_grad_(True)
    out = full(packed_input_ids=packed, cu_seqlens=cu, max_seqlen=16)
    (out * gout).sum().backward()

    with constants.model_scope("m"):
        model = ReaLModel(cfg, device="cpu", dtype=torch.float32,
                          tp_rank=g.tp_rank, tp_size=2)
        _fill_model_from_full(model, cfg, sd)
        opt = ZeRO1Optimizer(model, OptimizerConfig(
            lr=0.0, warmup_steps_proportion=0.0, gradient_clipping=0.0))
        opt.zero_grad()
        out = model(packed_input_ids=packed, cu_seqlens=cu, max_seqlen=16)
        v = cfg.vocab_size // 2
        (out * gout[:, g.tp_rank * v:(g.tp_rank + 1) * v]).sum().backward()
        opt.step()  # the optimizer's gradient reduction
        n_checked = 0
        for k in model.layout.keys:
            if not PL.grad_is_head_partial(k):
                continue
            got = model.grad_view(k)
            ref = full._params[k].grad
            assert ref.abs().max() > 1e-3, k
            torch.testing.assert_close(got, ref, atol=2e-4, rtol=2e-4)
            peer = [torch.empty_like(got) for _ in range(2)]
            dist.all_gather(peer, got.contiguous())
            assert torch.equal(peer[0], peer[1]), k
            n_checked += 1
        assert n_checked == 2 * cfg.n_layers
        # the other replicated gradients are still right (summed once)
        for k in ("1.attn.ln.weight", "2.mlp.ln.weight"):
            torch.testing.assert_close(model.grad_view(k), full._params[k].grad,
                                       atol=2e-4, rtol=2e-4)
    dist.barrier()


@pytest.mark.distributed
@pytest.mark.parametrize("sp", [False, True], ids=["tp2", "tp2-sp"])
def test_tp2_qk_ln_gradients_match_single(sp):
    LocalMultiProcessTest(2, _tp_grad_worker, sp).launch()
