"""Qwen3 (dense, 0.6B-32B) HF converters.

Qwen3 = llama tensor naming, an explicit head_dim (not hidden / heads), no
QKV bias by default, plus a plain-weight RMSNorm over head_dim on every q and
every k head before RoPE: `self_attn.q_norm` / `self_attn.k_norm`, one weight
[head_dim] each per layer (cfg.qk_rmsnorm, {i}.attn.q_ln / {i}.attn.k_ln).
Sliding-window variants and Qwen3-MoE are not covered."""
from typing import List

from realhf_amd.api.model import ReaLModelConfig
from realhf_amd.models.hf import HFFamily, register_family
from realhf_amd.models.hf import llama as L

_QK_NORMS = {
    "attn.q_ln.weight": "q_norm",
    "attn.k_ln.weight": "k_norm",
}


def hf_deps(cfg: ReaLModelConfig, key: str) -> List[str]:
    layer, name = key.split(".", 1)
    if name in _QK_NORMS:
        return [f"model.layers.{int(layer) - 1}.self_attn.{_QK_NORMS[name]}.weight"]
    return L.hf_deps(cfg, key)


def to_hf(cfg: ReaLModelConfig, sd):
    out = {}
    for k, v in sd.items():
        hfks = hf_deps(cfg, k)
        if not hfks:
            out[f"score.{k}"] = v  # critic head saved under a scoring name
            continue
        out[hfks[0]] = v
    return out


def config_from_hf(hf: dict) -> ReaLModelConfig:
    hf = dict(hf)
    if hf.get("use_sliding_window"):
        raise NotImplementedError("qwen3 with use_sliding_window")
    # transformers 5 keeps rope_theta (and the scaling) inside rope_parameters
    rp = hf.get("rope_parameters") or {}
    if hf.get("rope_theta") is None and rp.get("rope_theta") is not None:
        hf["rope_theta"] = rp["rope_theta"]
    if not hf.get("rope_scaling") and rp.get("rope_type") not in (None, "default"):
        hf["rope_scaling"] = {k: v for k, v in rp.items() if k != "rope_theta"}
    hf.setdefault("rope_theta", 1000000.0)
    hf.setdefault("rms_norm_eps", 1e-6)
    hf.setdefault("max_position_embeddings", 32768)
    cfg = L.config_from_hf(hf)  # head_dim, attention_bias (default False),
    # rms_norm_eps, tie_word_embeddings, rope_scaling types
    cfg.qk_rmsnorm = True
    return cfg


def config_to_hf(cfg: ReaLModelConfig) -> dict:
    out = L.config_to_hf(cfg)
    out["architectures"] = ["Qwen3ForCausalLM"]
    out["model_type"] = "qwen3"
    out["use_sliding_window"] = False
    return out


def make_test_config(**kw) -> ReaLModelConfig:
    kw.setdefault("qk_rmsnorm", True)
    kw.setdefault("layer_norm_epsilon", 1e-6)
    return L.make_test_config(**kw)


register_family(
    HFFamily(
        name="qwen3",
        hf_arch="Qwen3ForCausalLM",
        hf_deps=hf_deps,
        from_hf=L.from_hf,
        to_hf=to_hf,
        config_from_hf=config_from_hf,
        config_to_hf=config_to_hf,
        make_test_config=make_test_config,
    )
)
