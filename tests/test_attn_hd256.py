"""head_dim 256 (gemma) — the parts that need no GPU: the one head-dim gate
of the HIP attention kernels, and the reference path at 256 vs HuggingFace."""
import inspect

import numpy as np
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.models import generation, layers
from realhf_amd.models.real_model import ReaLModel
from realhf_amd.ops import functional as F
from realhf_amd.parallel import pp


def test_hip_attn_head_dims_constant():
    assert F.HIP_ATTN_HEAD_DIMS == (64, 128, 256)


def test_decode_graph_predicate_accepts_256():
    """generate()'s hipGraph gate: bf16 on a GPU at every kernel head dim;
    never on the CPU, in fp16 or at a head dim without a kernel."""
    fam = hf_reg.get_family("gemma")
    ok = generation.decode_graph_supported
    for hd in F.HIP_ATTN_HEAD_DIMS:
        cfg = fam.make_test_config(head_dim=hd)
        assert ok(cfg, torch.bfloat16, torch.device("cuda", 0))
        assert ok(cfg, torch.bfloat16, "cuda")
        assert not ok(cfg, torch.bfloat16, torch.device("cpu"))
        assert not ok(cfg, torch.float16, torch.device("cuda", 0))
    assert not ok(fam.make_test_config(head_dim=96), torch.bfloat16,
                  torch.device("cuda", 0))


def test_no_private_head_dim_tuples():
    """The fused-decode gate (layers), the graph gates (generation, pp) and
    the op dispatch all read F.HIP_ATTN_HEAD_DIMS; none keeps a (64, 128)
    of its own."""
    for mod in (layers, generation, pp, F):
        src = inspect.getsource(mod)
        assert "(64, 128)" not in src, mod.__name__
        assert ("HIP_ATTN_HEAD_DIMS" in src
                or "decode_graph_supported" in src), mod.__name__


def _gemma256():
    fam = hf_reg.get_family("gemma")
    cfg = fam.make_test_config(n_layers=2, hidden_dim=64, n_heads=2,
                               n_kv_heads=1, head_dim=256, vocab_size=64)
    cfg.dtype = "float32"
    return fam, cfg


def _hf_model(fam, cfg):
    import transformers

    d = dict(fam.config_to_hf(cfg))
    hf_cfg = transformers.AutoConfig.for_model(d.pop("model_type"), **d)
    torch.manual_seed(42)
    return transformers.AutoModelForCausalLM.from_config(hf_cfg).eval().float()


def test_gemma_hd256_cpu_forward_backward_matches_hf():
    """The reference path at head_dim 256 with 2 query heads on 1 kv head
    (gemma-2b's shape class): packed logits and parameter gradients vs
    transformers, at test_model_cpu's tolerances."""
    fam, cfg = _gemma256()
    hf_model = _hf_model(fam, cfg)
    assert hf_model.config.head_dim == 256
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    hf_reg.load_from_hf_state_dict(model, "gemma", hf_model.state_dict())
    for p in model._params.values():
        p.requires_grad_(True)

    rng = np.random.RandomState(0)
    lens = [5, 19, 12]
    ids = [torch.from_numpy(rng.randint(0, cfg.vocab_size, size=l)).long()
           for l in lens]
    packed = torch.cat(ids)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)

    ours = model(packed_input_ids=packed, cu_seqlens=cu, max_seqlen=max(lens))
    ours_lp = torch.log_softmax(ours.float(), -1)
    ref_lp = torch.cat([
        torch.log_softmax(hf_model(input_ids=x.unsqueeze(0)).logits[0].float(), -1)
        for x in ids])
    torch.testing.assert_close(ours_lp, ref_lp, atol=2e-4, rtol=2e-3)

    # backward of the same scalar through both models
    w = torch.from_numpy(rng.randn(*ours_lp.shape)).float()
    (ours_lp * w).sum().backward()
    (ref_lp * w).sum().backward()
    hf_p = dict(hf_model.named_parameters())
    for ours_k, hf_k in (
        # upstream of both attention layers: these carry dQ, dK and dV
        ("0.wte.weight", "model.embed_tokens.weight"),
        ("1.attn.ln.weight", "model.layers.0.input_layernorm.weight"),
        ("2.attn.ln.weight", "model.layers.1.input_layernorm.weight"),
        ("1.attn.wo.weight", "model.layers.0.self_attn.o_proj.weight"),
        ("1.mlp.down.weight", "model.layers.0.mlp.down_proj.weight"),
    ):
        g, r = model._params[ours_k].grad, hf_p[hf_k].grad
        assert g is not None and torch.isfinite(g).all()
        if ours_k == "0.wte.weight":
            # transformers treats token 0 as padding_idx: its embedding
            # row gets no input-side gradient there
            g, r = g[1:], r[1:]
        torch.testing.assert_close(g, r, atol=2e-4 * float(r.abs().max()),
                                   rtol=2e-3)
