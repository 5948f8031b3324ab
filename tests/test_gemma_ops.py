"""Gemma's GeGLU op — the parts that need no GPU: the torch reference is the
expression the MLP used to compute inline, bit for bit, and routing the MLP
through ops.geglu changes no CPU result."""
import numpy as np
import pytest
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.models import layers
from realhf_amd.models.real_model import ReaLModel
from realhf_amd.ops import functional as F


def _inline_geglu(gu):
    """The GeGLU branch of ReaLModelBlock._mlp_body before ops.geglu."""
    gate, up = gu.chunk(2, dim=-1)
    return (
        torch.nn.functional.gelu(gate.float(), approximate="tanh") * up.float()
    ).to(gu.dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_geglu_ref_is_the_inline_expression(dtype):
    torch.manual_seed(0)
    gu = (torch.randn(37, 2 * 48) * 3).to(dtype)
    gu[0, :8] = torch.tensor([-30, -12, -6, -0.0, 0, 6, 12, 30]).to(dtype)
    assert torch.equal(F.geglu_ref(gu), _inline_geglu(gu))
    # a non-contiguous view, as the last dim of a wider buffer
    wide = torch.cat([gu, gu], dim=-1)[:, : 2 * 48]
    assert torch.equal(F.geglu_ref(wide), _inline_geglu(gu))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_geglu_on_cpu_is_the_reference(dtype, monkeypatch):
    torch.manual_seed(1)
    gu = (torch.randn(5, 32) * 3).to(dtype)
    want = F.geglu_ref(gu)
    assert torch.equal(F.geglu(gu), want)
    monkeypatch.setenv("REALHF_AMD_NO_GEMMA_OPS", "1")
    assert F.gemma_ops_enabled() is False
    assert torch.equal(F.geglu(gu), want)
    monkeypatch.delenv("REALHF_AMD_NO_GEMMA_OPS")
    assert F.gemma_ops_enabled() is True


def test_geglu_ref_gradient_is_the_inline_gradient():
    torch.manual_seed(2)
    gu = torch.randn(9, 64) * 3
    g = torch.randn(9, 32)
    a = gu.clone().requires_grad_(True)
    b = gu.clone().requires_grad_(True)
    F.geglu(a).backward(g)
    _inline_geglu(b).backward(g)
    assert torch.equal(a.grad, b.grad)


def _run_gemma(monkeypatch, geglu):
    fam = hf_reg.get_family("gemma")
    cfg = fam.make_test_config()
    cfg.dtype = "float32"
    model = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    torch.manual_seed(3)
    model.random_init()
    with torch.no_grad():  # norm weights off their init value
        for k, t in model._params.items():
            if t.ndim == 1:
                t.add_(0.1 * torch.randn_like(t))
    model.allocate_grad_buffer()
    for k, p in model._params.items():
        p.requires_grad_(True)
        p.grad = model.grad_view(k)
    if geglu is not None:
        monkeypatch.setattr(layers.ops, "geglu", geglu)
    rng = np.random.RandomState(0)
    lens = [5, 19, 12]
    packed = torch.from_numpy(rng.randint(0, cfg.vocab_size, size=sum(lens))).long()
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    logits = model(packed_input_ids=packed, cu_seqlens=cu, max_seqlen=max(lens))
    w = torch.from_numpy(rng.randn(*logits.shape)).float()
    (torch.log_softmax(logits.float(), -1) * w).sum().backward()
    return logits.detach(), model.flat_grad.clone()


def test_gemma_cpu_model_unchanged_by_the_geglu_op(monkeypatch):
    """Forward and backward of the CPU gemma test model through ops.geglu
    equal those with the old inline math, bit for bit."""
    calls = []

    def inline(gu):
        calls.append(1)
        return _inline_geglu(gu)

    logits, grad = _run_gemma(monkeypatch, None)
    logits_old, grad_old = _run_gemma(monkeypatch, inline)
    assert calls, "the MLP did not go through ops.geglu"
    assert grad.abs().sum() > 0
    assert torch.equal(logits, logits_old)
    assert torch.equal(grad, grad_old)
