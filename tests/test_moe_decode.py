"""MoE decode, CPU side: moe_decode_ref is MoELayer.forward in eval mode, and
moe_decode_supported refuses every excluded configuration."""
import dataclasses

import pytest
import torch

from realhf_amd.models.hf import get_family
from realhf_amd.ops import functional as ops


def _cfg(**moe_kw):
    cfg = get_family("mixtral").make_test_config(
        n_layers=1, hidden_dim=64, n_heads=2, n_kv_heads=2, head_dim=32,
        vocab_size=64, intermediate_dim=128,
    )
    cfg.moe = dataclasses.replace(cfg.moe, **moe_kw)
    return cfg


@pytest.mark.parametrize("norm_topk", [True, False])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 2)])
def test_ref_matches_layer_forward(E, k, norm_topk):
    from realhf_amd.models.moe import MoELayer

    cfg = _cfg(num_experts=E, top_k=k, norm_topk_prob=norm_topk)
    H, I = cfg.hidden_dim, cfg.intermediate_dim
    torch.manual_seed(0)
    wg, wu = torch.randn(2, E, I, H) / H ** 0.5
    wd = torch.randn(E, H, I) / I ** 0.5
    rw = 4 * torch.randn(E, H) / H ** 0.5
    params = {"1.mlp.router.weight": rw}
    for e in range(E):
        for part, w in (("gate", wg), ("up", wu), ("down", wd)):
            params[f"1.mlp.experts.{e}.{part}.weight"] = w[e]
    layer = MoELayer(cfg, 1, params, tp_size=1).eval()
    h = torch.randn(5, H)
    res = torch.randn(5, H)
    with torch.no_grad():
        want = res + layer(h)
        assert torch.equal(layer.decode(h, residual=res), want)  # CPU: forward
    got = ops.moe_decode_ref(h, rw, wg, wu, wd, k, norm_topk, residual=res)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    assert torch.equal(ops.moe_decode(h, rw, wg, wu, wd, k, norm_topk, res), got)


@pytest.mark.parametrize("case", ["cpu", "fp32", "capacity", "ep", "tp", "gelu",
                                  "idim96", "kill"])
def test_supported_refuses(case, monkeypatch):
    monkeypatch.delenv("REALHF_AMD_NO_MOE_DECODE", raising=False)
    cfg = _cfg()
    args = dict(dtype=torch.bfloat16, device="cuda", tp=1, ep=1)
    assert ops.moe_decode_supported(cfg, **args)
    if case == "cpu":
        args["device"] = "cpu"
    elif case == "fp32":
        args["dtype"] = torch.float32
    elif case == "capacity":
        cfg = _cfg(capacity_factor=1.5)
    elif case in ("ep", "tp"):
        args[case] = 2
    elif case == "gelu":
        cfg.activation = "gelu"
    elif case == "idim96":
        cfg.intermediate_dim = 96
    else:
        monkeypatch.setenv("REALHF_AMD_NO_MOE_DECODE", "1")
    assert not ops.moe_decode_supported(cfg, **args)
