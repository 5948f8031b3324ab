"""FP8 expert weights off the GPU: ops.moe_decode(fp8=...) and the expert
pairs that Fp8DecodeWeights holds, refreshes and drops for a tiny mixtral."""
import math

import pytest
import torch

from realhf_amd.ops import functional as ops


def test_moe_decode_fp8_is_ref_on_dequantised_stacks():
    torch.manual_seed(0)
    M, H, I, E, k = 5, 64, 128, 4, 2
    h, res = torch.randn(M, H), torch.randn(M, H)
    rw = 4 * torch.randn(E, H) / math.sqrt(H)
    stacks = [torch.randn(E, n, kk) / math.sqrt(kk)
              for n, kk in ((I, H), (I, H), (H, I))]
    fp8 = tuple(ops.quantize_rows_e4m3(w) for w in stacks)
    deq = [q.float() * s[..., None] for q, s in fp8]
    want = ops.moe_decode_ref(h, rw, *deq, k, True, residual=res)
    got = ops.moe_decode(h, rw, *stacks, k, True, residual=res, fp8=fp8)
    assert torch.equal(got, want)


@pytest.mark.parametrize("bs,kill,held", [(16, None, True), (17, None, False),
                                          (3, "1", False)])
def test_fp8_decode_weights_expert_pairs(monkeypatch, bs, kill, held):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.generation import Fp8DecodeWeights, _session_key
    from realhf_amd.models.real_model import ReaLModel

    monkeypatch.delenv("REALHF_AMD_NO_FP8_MOE", raising=False)
    cfg = hf_reg.get_family("mixtral").make_test_config(
        n_layers=2, hidden_dim=128, n_heads=2, n_kv_heads=2, head_dim=64,
        vocab_size=64, intermediate_dim=64)
    cfg.family = "mixtral"
    torch.manual_seed(0)
    m = ReaLModel(cfg, device="cpu", dtype=torch.bfloat16)
    m.random_init(std=0.05)
    key = _session_key(m, bs, 128, "fp8_e4m3")
    if kill:
        monkeypatch.setenv("REALHF_AMD_NO_FP8_MOE", kill)
        assert _session_key(m, bs, 128, "fp8_e4m3") != key
    fp8 = Fp8DecodeWeights(m, bs)
    dense = sum(q.numel() + 4 * s.numel() for d in fp8.pairs for q, s in d.values())
    if not held:
        assert fp8.expert_pairs == [(), ()] and fp8.nbytes() == dense
        return
    fp8.refresh()
    E, H, I = cfg.moe.num_experts, cfg.hidden_dim, cfg.intermediate_dim
    assert fp8.nbytes() == dense + 2 * (3 * E * H * I + 4 * E * (2 * I + H))
    for blk, ep in zip(fp8.blocks, fp8.expert_pairs):
        for (q, s), w in zip(ep, blk.moe.decode_stacks()):
            for e in range(E):
                q_ref, s_ref = ops.quantize_rows_e4m3_ref(w[e])
                assert torch.equal(q[e].view(torch.uint8), q_ref.view(torch.uint8))
                assert torch.equal(s[e], s_ref)
        with fp8.installed():
            assert blk.moe.fp8 is ep
        assert blk.moe.fp8 == ()
