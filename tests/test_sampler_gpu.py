"""The sample_logits kernel against sample_logits_ref evaluated in fp64 on
the CPU from the same 16- or 32-bit logits: tokens and masks exactly,
log-probs to 1e-4 (fp32 against fp64 on |logits| <= 30 is an lse error of
a few 1e-6), two calls bitwise equal.

Exact tokens are fair because every case builds its own top_p and u from
the fp64 CDF: top_p is the midpoint between two adjacent exclusive prefix
masses, u the midpoint of a chosen candidate's interval, and every such
gap is asserted to be >= GAP = 2e-3 before the kernel runs; fp32 prefix
sums over <= 1024 terms move a normalised mass by about 1024 * 2^-24 =
6e-5.  Rows are a permuted profile, ten heavy values 0.5 apart over a tail
16 below them, plus noise; a bad seed fails the margin assert."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C  # noqa: E402,F401 — must exist on a GPU box

GAP = 2e-3
LOGP_TOL = 1e-4
bf16, fp32 = torch.bfloat16, torch.float32


def _rows(bs, V, dtype, T, seed=0):
    """[bs, V] logits whose x = logits / T is the profile above."""
    g = torch.Generator().manual_seed(seed)
    prof = torch.cat([8 - 0.5 * torch.arange(10.),
                      -30 + 14 * torch.rand(V - 10, generator=g)])
    x = torch.stack([prof[torch.randperm(V, generator=g)] for _ in range(bs)])
    x += 0.01 * torch.randn(bs, V, generator=g)
    return (x * T).to(dtype)


def _plan(logits, T, k, cut):
    """(top_p, u [bs] fp32, expected token per row) from the fp64 CDF in the
    reference's candidate order; cut = kept candidates, None = no top_p."""
    x = logits.cpu().double() / T
    bs, V = x.shape
    if k >= V and cut is None:  # full form: index order
        vals, order = x, torch.arange(V).expand(bs, V)
    else:
        vals, order = torch.sort(x, dim=-1, descending=True, stable=True)
        vals, order = vals[:, :k], order[:, :k]
    e = (vals - x.amax(-1, keepdim=True)).exp()
    cum = e.cumsum(-1)
    if cut is None:
        top_p = 1.0
        m = (vals > float("-inf")).sum(-1)
        z2 = cum[:, -1]
    else:
        pex = (cum - e) / cum[:, -1:]
        lo, hi = pex[:, cut - 1].max().item(), pex[:, cut].min().item()
        assert hi - lo >= GAP, (lo, hi)
        top_p = (lo + hi) / 2
        m = torch.full((bs,), cut)
        z2 = cum[:, cut - 1]
    u, want = [], []
    for r in range(bs):  # first, second, a middle and the last drawable one
        ok = (e[r] / z2[r] >= GAP).nonzero()[:, 0]
        ok = ok[ok < m[r]] if vals is not x else ok
        assert ok.numel() >= 1 and (vals is x or ok[-1] == m[r] - 1)
        pos = ok[[0, 1, ok.numel() // 2, -1][r % 4] % ok.numel()]
        u.append((cum[r, pos] - e[r, pos] / 2) / z2[r])
        want.append(order[r, pos])
    return top_p, torch.stack(u).float(), torch.stack(want)


def _check(logits, u, T, k, top_p, greedy, want_mask, want_tok=None):
    ref = F.sample_logits_ref(logits.cpu().double(), u.double(), T, k, top_p,
                              greedy, want_mask)
    if want_tok is not None:  # the plan and the reference agree
        assert torch.equal(ref[0], want_tok)
    assert F.sample_logits_unsupported(logits, k, top_p, greedy) is None
    got = F.sample_logits(logits.cuda(), u.cuda(), T, k, top_p, greedy, want_mask)
    again = F.sample_logits(logits.cuda(), u.cuda(), T, k, top_p, greedy, want_mask)
    torch.cuda.synchronize()
    err = (got[1].cpu().double() - ref[1]).abs().max().item()
    print("tokens", got[0].tolist()[:4], "max |dlogp|", err)
    assert got[0].dtype == torch.int64 and torch.equal(got[0].cpu(), ref[0])
    assert err <= LOGP_TOL
    assert (got[2] is None) == (ref[2] is None)
    if ref[2] is not None:
        assert got[2].dtype == torch.bool and torch.equal(got[2].cpu(), ref[2])
        assert torch.equal(got[2], again[2])
    assert torch.equal(got[0], again[0])
    assert torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))


# k: 0 = off (V); cut: candidates top_p keeps, None = top_p 1
@pytest.mark.parametrize("bs,V,dtype,k,cut,T,want_mask", [
    (1, 1031, fp32, 1024, 7, 1.0, True),      # V just above k; a partial sweep
    (16, 2056, bf16, 1000, 7, 0.7, False),
    (16, 2056, fp32, 1, None, 1.0, True),
    (16, 32000, bf16, 1000, 7, 1.0, True),    # the bench row
    (16, 32000, bf16, 5, None, 0.7, False),
    (2, 50257, bf16, 1000, 6, 1.0, True),     # second row off the 16-byte grid
    (2, 50257, fp32, 1024, 7, 0.7, True),     # fp32 beyond the registers
    (2, 262144, bf16, 1000, 7, 1.0, True),    # re-read per pass
    (2, 262144, fp32, 5, None, 0.7, False),
    (1, 1031, fp32, 0, None, 0.7, False),     # full form
    (16, 32000, bf16, 0, None, 1.0, True),
    (2, 50257, bf16, 50257, None, 1.0, False),
    (2, 262144, fp32, 0, None, 1.0, True),
    (16, 32000, bf16, "greedy", None, 1.0, False),
    (1, 2056, fp32, "greedy", None, 0.7, False),
    (2, 262144, bf16, "greedy", None, 1.0, False),
])
def test_kernel_matches_fp64_reference(bs, V, dtype, k, cut, T, want_mask):
    logits = _rows(bs, V, dtype, T)
    if k == "greedy":
        _check(logits, torch.zeros(bs), T, 0, 1.0, True, False)
        return
    top_p, u, want = _plan(logits, T, k or V, cut)
    _check(logits, u, T, k, top_p, False, want_mask, want)


def test_ties_and_minus_inf():
    """k = 5 over 8, 7.5, 7, 6.5 and three 6s: the lowest-index 6 is the
    fifth candidate.  Column 3 is -inf everywhere; row 2 ends in a run of
    -inf that leaves 3 finite entries, fewer than k."""
    V = 2056
    logits = _rows(3, V, bf16, 1.0, seed=1).clamp(max=-16.0)
    for r, at in enumerate(([900, 17, 2055, 5, 1300, 40, 1299],
                            [0, 1, 2, 4, 2054, 2050, 9])):
        logits[r, at] = torch.tensor([8, 7.5, 7, 6.5, 6, 6, 6], dtype=bf16)
    logits[2, :3] = torch.tensor([7, 8, 7.5], dtype=bf16)
    logits[2, 4:] = float("-inf")
    logits[:, 3] = float("-inf")
    # every row draws its last kept candidate: the middle of its interval
    e = torch.tensor([0, -.5, -1, -1.5, -2]).double().exp()
    assert e[4] / e.sum() >= GAP and e[2] / e[:3].sum() >= GAP
    last5 = 1 - e[4] / 2 / e.sum()
    u = torch.stack([last5, last5, 1 - e[2] / 2 / e[:3].sum()]).float()
    _check(logits, u, 1.0, 5, 1.0, False, True)
    tok = F.sample_logits(logits.cuda(), u.cuda(), 1.0, 5, 1.0, False, True)[0]
    assert tok.tolist() == [40, 9, 0]
    # the same rows through the full form: -inf is masked, never drawn
    top_p, u, want = _plan(logits, 1.0, V, None)
    _check(logits, u, 1.0, 0, 1.0, False, True, want)


def test_generate_with_hip_sampler(monkeypatch):
    """Tiny llama, prefill + 8 steps, 3 sequences: sampler="hip" yields the
    tokens, log-probs and logits mask that sample_logits_ref gives on the
    logits the model produced, with the uniforms of the same seed."""
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models import generation as genmod
    from realhf_amd.models.real_model import ReaLModel

    monkeypatch.delenv("REALHF_AMD_GEN_SAMPLER", raising=False)
    STEPS = 8
    cfg = hf_reg.get_family("llama").make_test_config(  # test_fp8_decode_gpu's
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=2, head_dim=128,
        vocab_size=256, intermediate_dim=512)
    cfg.family = "llama"
    torch.manual_seed(44)
    m = ReaLModel(cfg, device="cuda", dtype=bf16)
    m.random_init(std=0.05)
    toks = torch.randint(0, 256, (26,), generator=torch.Generator().manual_seed(1))
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    seen = []
    real = F.sample_logits
    monkeypatch.setattr(genmod.ops, "sample_logits", lambda logits, *a, **kw: (
        seen.append(logits.clone()), real(logits, *a, **kw))[1])
    g = GenerationHyperparameters(max_new_tokens=STEPS + 1, top_k=5, top_p=0.9,
                                  sampler="hip", force_no_logits_mask=False)
    out = genmod.generate(m, toks.cuda(), cu.cuda(), g,
                          generator=torch.Generator("cuda").manual_seed(7))
    assert len(seen) == STEPS + 1 and seen[0].dtype == bf16
    assert m._gen_session[1].decoder.graph is not None
    gen = torch.Generator("cuda").manual_seed(7)
    for t, logits in enumerate(seen):
        u = torch.rand(3, generator=gen, device="cuda")
        tok, logp, mask = F.sample_logits_ref(logits.cpu().double(),
                                              u.cpu().double(), 1.0, 5, 0.9,
                                              False, True)
        assert torch.equal(out.gen_tokens[:, t].cpu(), tok)
        assert (out.gen_logprobs[:, t].cpu().double() - logp).abs().max() <= LOGP_TOL
        assert torch.equal(out.logits_mask[:, t].cpu(), mask)
