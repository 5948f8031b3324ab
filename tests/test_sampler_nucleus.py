"""The sampler kernel's gate with the search form: what is left is the dtype
and top_k > 1024 over rows beyond the registers, where it measured slower."""
import pytest
import torch

from realhf_amd.ops import functional as F


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (2000, 1.0)])
def test_gate_takes_every_filter(top_k, top_p):
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.zeros(2, 32000, dtype=dtype)
        assert F.sample_logits_unsupported(x, top_k, top_p, False) is None
    assert isinstance(F.sample_logits_unsupported(x.half(), top_k, top_p, False), str)
    long_row = torch.zeros(1, 128256, dtype=torch.bfloat16)
    assert F.sample_logits_unsupported(long_row, 0, 0.9, False) is None
    assert isinstance(F.sample_logits_unsupported(long_row, 4000, 0.9, False), str)
