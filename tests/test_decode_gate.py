"""The one gate of the fused decode block, without a GPU: the truth table of
generation's weight_quant / kv_quant blockers and their agreement with
layers.fused_decode_blocker, the HIP-attention predicate behind
decode_graph_supported, and the skinny GEMMs' split-K rule."""
import itertools
import types

import pytest
import torch

from realhf_amd.models import generation as genmod
from realhf_amd.models import layers
from realhf_amd.ops import functional as F

NO_FUSED = "REALHF_AMD_NO_FUSED_DECODE"
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
HEAD_DIMS = (64, 96, 128, 256)


def _stub(lora, qk_layernorm, head_dim, dtype, is_cuda, pp_size):
    """What the blockers read of a model."""
    return types.SimpleNamespace(
        config=types.SimpleNamespace(qk_layernorm=qk_layernorm,
                                     head_dim=head_dim),
        lora_flat=object() if lora else None, dtype=dtype, pp_size=pp_size,
        flat_param=types.SimpleNamespace(is_cuda=is_cuda))


def _expected(which, lora, qk_layernorm, head_dim, dtype, is_cuda, no_fused,
              pp_size):
    """The keyword of the first reason the blocker gives, None if it gives
    none: the two blockers as they stood before they shared one gate, clause
    by clause and in their order.  They differ in the dtype clause only."""
    if lora:
        return "LoRA"
    if qk_layernorm:
        return "qk_layernorm"
    if head_dim not in (64, 128, 256):
        return f"head_dim {head_dim}"
    if dtype != torch.bfloat16 and (which == "weight" or is_cuda):
        return str(dtype)
    if no_fused:
        return "NO_FUSED_DECODE"
    if pp_size > 1:
        return "pp > 1"
    return None


def _cases():
    return itertools.product((False, True), (False, True), HEAD_DIMS, DTYPES,
                             (False, True), (1, 2))


@pytest.mark.parametrize("no_fused", [False, True])
def test_blockers_truth_table(monkeypatch, no_fused):
    """All 384 combinations of LoRA, qk_layernorm, head dim, dtype, device,
    REALHF_AMD_NO_FUSED_DECODE and pp size, for both blockers."""
    monkeypatch.delenv(NO_FUSED, raising=False)
    if no_fused:
        monkeypatch.setenv(NO_FUSED, "1")
    n = 0
    for lora, qk, hd, dtype, is_cuda, pp in _cases():
        m = _stub(lora, qk, hd, dtype, is_cuda, pp)
        for which, blocker in (("weight", genmod.weight_quant_blocker),
                               ("kv", genmod.kv_quant_blocker)):
            want = _expected(which, lora, qk, hd, dtype, is_cuda, no_fused, pp)
            got = blocker(m)
            case = (which, lora, qk, hd, dtype, is_cuda, no_fused, pp)
            if want is None:
                assert got is None, case
            else:
                assert got is not None and want in got, (case, got)
                if which == "weight" and want == str(dtype):
                    assert "bfloat16" in got, (case, got)
        n += 1
    assert n == 192  # x 2 settings of the variable


@pytest.mark.parametrize("no_fused", [False, True])
def test_kv_blocker_agrees_with_the_block_gate(monkeypatch, no_fused):
    """Without pp, a GPU model may use the FP8 KV cache exactly when its
    blocks' dispatcher takes the fused decode block, its only writer there.
    (On the CPU fused_decode_blocker always names a reason and the torch
    references serve the cache; there the blocker is the gate asked as for a
    bf16 GPU model.)"""
    monkeypatch.delenv(NO_FUSED, raising=False)
    if no_fused:
        monkeypatch.setenv(NO_FUSED, "1")
    for lora, qk, hd, dtype, is_cuda, pp in _cases():
        if pp != 1:
            continue
        m = _stub(lora, qk, hd, dtype, is_cuda, pp)
        kv_ok = genmod.kv_quant_blocker(m) is None
        gate = layers.fused_decode_blocker(m.config, dtype, is_cuda, lora)
        case = (lora, qk, hd, dtype, is_cuda, no_fused)
        assert (kv_ok == (gate is None)) or not is_cuda, case
        if not is_cuda:
            assert gate is not None, case
            assert kv_ok == (layers.fused_decode_blocker(
                m.config, torch.bfloat16, True, lora) is None), case
        # and FP8 weights exactly when the gate would open on the GPU
        assert (genmod.weight_quant_blocker(m) is None) == (
            layers.fused_decode_blocker(m.config, dtype, True, lora) is None
        ), case


# (dtype, device type, head dim) the HIP attention kernels take; every other
# point of the grid is False
HIP_ATTN_TRUE = {
    (torch.bfloat16, "cuda", 64),
    (torch.bfloat16, "cuda", 128),
    (torch.bfloat16, "cuda", 256),
}


def test_decode_graph_supported_grid():
    n_true = 0
    for dtype, dev, hd in itertools.product(DTYPES, ("cuda", "cpu"), HEAD_DIMS):
        cfg = types.SimpleNamespace(head_dim=hd)
        want = (dtype, dev, hd) in HIP_ATTN_TRUE
        for device in (dev, torch.device(dev), torch.device(dev, 0)):
            got = genmod.decode_graph_supported(cfg, dtype, device)
            assert got is want, (dtype, device, hd)
        n_true += want
    assert n_true == 3


def test_hip_attn_supported_grid():
    for dtype, dev, hd in itertools.product(DTYPES, ("cuda", "cpu"), HEAD_DIMS):
        want = (dtype, dev, hd) in HIP_ATTN_TRUE
        for device in (dev, torch.device(dev), torch.device(dev, 0)):
            assert F.hip_attn_supported(dtype, hd, device) is want, (
                dtype, device, hd)


def test_skinny_splitk_rule(monkeypatch):
    """8, doubled while K // splitk exceeds the slice cap (default 1024)."""
    monkeypatch.delenv("REALHF_AMD_SG_KSLICE", raising=False)
    monkeypatch.setattr(F, "_SG_KSLICE", None)  # the cap is read once
    got = [F.skinny_splitk(K) for K in (4096, 8192, 11008, 14336, 32768)]
    assert got == [8, 8, 16, 16, 32]
