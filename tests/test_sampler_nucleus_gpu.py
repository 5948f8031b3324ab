"""The sampler's search form (top_p without top_k, top_k > 1024) against
sample_logits_ref in fp64 on the CPU: tokens and masks exactly, log-probs to
1e-4, two calls bitwise equal.  Margins come from the fp64 CDF alone: top_p
is the midpoint between the exclusive prefix masses of candidates cut-1 and
cut, u the midpoint of a kept candidate's interval, each gap asserted >= 2e-4
of normalised mass (the kernel's deviation is estimated at a few 1e-6).
"plateau" rows, 2048 values in [4, 4.5), are about 16 distinct bf16 values."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box
from realhf_amd.api.model import GenerationHyperparameters  # noqa: E402
from realhf_amd.models import generation as genmod, hf as hf_reg  # noqa: E402
from realhf_amd.models.real_model import ReaLModel  # noqa: E402
from realhf_amd.ops import functional as F  # noqa: E402
from tests.test_sampler_gpu import _check, bf16, fp32  # noqa: E402

GAP = 2e-4


def _rows(bs, V, dtype, T, plateau):
    g = torch.Generator().manual_seed(0)  # heavy: test_sampler_gpu's profile
    top = 4 + 0.5 * torch.rand(2048, generator=g) if plateau else 8 - 0.5 * torch.arange(10.)
    prof = torch.cat([top, -30 + 14 * torch.rand(V - top.numel(), generator=g)])
    x = torch.stack([prof[torch.randperm(V, generator=g)] for _ in range(bs)])
    if not plateau:
        x += 0.01 * torch.randn(bs, V, generator=g)
    return (x * T).to(dtype)


def _plan(logits, T, k, cut):
    """(top_p, u [bs] fp32, expected tokens) from the fp64 CDF."""
    vals, order = torch.sort(logits.double() / T, dim=-1, descending=True, stable=True)
    vals, order = vals[:, :k], order[:, :k]
    e = (vals - vals[:, :1]).exp()
    cum = e.cumsum(-1)
    m, top_p = (vals > float("-inf")).sum(-1), 1.0
    if cut is not None:
        pex = (cum - e) / cum[:, -1:]
        lo, hi = pex[:, cut - 1].max().item(), pex[:, cut].min().item()
        assert hi - lo >= GAP, (lo, hi)
        m, top_p = torch.full_like(m, cut), (lo + hi) / 2
    u, want = [], []
    for r in range(len(m)):  # first, second, a middle and the last kept one
        z2 = cum[r, m[r] - 1]
        ok = (e[r, :m[r]] / z2 >= GAP).nonzero()[:, 0]
        assert ok[-1] == m[r] - 1
        pos = ok[[0, 1, ok.numel() // 2, -1][r % 4] % ok.numel()]
        u.append((cum[r, pos] - e[r, pos] / 2) / z2)
        want.append(order[r, pos])
    return top_p, torch.stack(u).float(), torch.stack(want)


@pytest.mark.parametrize("bs,V,dtype,k,cut,T,plateau,want_mask", [  # k 0: off
    (1, 1031, fp32, 0, 7, 1.0, False, True),       # smallest; a partial sweep
    (16, 32000, bf16, 0, 7, 0.7, False, False),    # the common configuration
    (16, 32000, bf16, 0, 1500, 1.0, True, True),   # more kept than the sort holds
    (2, 50257, fp32, 0, 1500, 0.7, True, True),    # off the 16-byte grid, no registers
    (2, 262144, bf16, 0, 1500, 1.0, True, True),   # re-read per pass
    (2, 2056, fp32, 1025, None, 1.0, True, False),  # just past the select form
    (2, 32000, bf16, 2000, None, 1.0, True, True),  # rank threshold inside a tie run
    (2, 50257, bf16, 3000, 1500, 0.7, True, True),  # rank, then cut, then draw
    (2, 1000, bf16, 0, 7, 1.0, False, True),       # V <= 1024: the select form, k = V
])
def test_search_form_matches_fp64_reference(bs, V, dtype, k, cut, T, plateau, want_mask):
    logits = _rows(bs, V, dtype, T, plateau)
    top_p, u, want = _plan(logits, T, k or V, cut)
    _check(logits, u, T, k, top_p, False, want_mask, want)


def test_ties_and_minus_inf():
    """All-equal rows, where integer mass is exact: indices 0..1028 are kept;
    then column 3 at -inf; then 4 finite entries under top_k = 2000."""
    V = 2056
    logits = torch.full((2, V), 1.5)
    u = torch.tensor([0.25 + 0.5 / 1029, 0.9995])
    _check(logits, u, 1.0, 0, 1028.5 / V, False, True)
    tok, _, mask = F.sample_logits(logits.cuda(), u.cuda(), 1.0, 0, 1028.5 / V, False, True)
    assert tok.tolist() == [257, 1028] and (~mask).sum(-1).tolist() == [1029, 1029]
    logits[:, 3] = float("-inf")
    _check(logits, u, 1.0, 0, 1028.5 / V, False, True)
    logits = _rows(2, V, fp32, 1.0, True)
    logits[:, 4:] = float("-inf")
    _, u, want = _plan(logits, 1.0, 2000, None)
    _check(logits, u, 1.0, 2000, 1.0, False, True, want)


def test_generate_nucleus_runs_the_kernel(monkeypatch):
    """A tiny llama, top_p 0.9 without top_k: every step is one kernel call,
    no fallback is logged, and generate() returns the op's results."""
    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=2, head_dim=128,
        vocab_size=2056, intermediate_dim=512)
    cfg.family = "llama"
    torch.manual_seed(44)
    m = ReaLModel(cfg, device="cuda", dtype=bf16)
    m.random_init(std=0.05)
    toks = torch.randint(0, 2056, (26,), generator=torch.Generator().manual_seed(1))
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    seen, real = [], C.sample_logits
    monkeypatch.setattr(C, "sample_logits", lambda logits, *a, **kw: (
        seen.append(logits.clone()), real(logits, *a, **kw))[1])
    g = GenerationHyperparameters(max_new_tokens=9, top_k=0, top_p=0.9,
                                  sampler="hip", force_no_logits_mask=False)
    out = genmod.generate(m, toks.cuda(), cu.cuda(), g,
                          generator=torch.Generator("cuda").manual_seed(7))
    assert len(seen) == 9 and not getattr(m, "_sampler_warned", False)
    gen = torch.Generator("cuda").manual_seed(7)
    for t, logits in enumerate(list(seen)):  # the op below is recorded too
        u = torch.rand(3, generator=gen, device="cuda")
        want = F.sample_logits(logits, u, 1.0, 0, 0.9, False, True)
        for a, b in zip((out.gen_tokens, out.gen_logprobs, out.logits_mask), want):
            assert torch.equal(a[:, t], b)
