"""Fused vocab log-prob HIP kernels (ops/csrc/logprob.hip) against the
fp32 torch oracle.  Shapes are the smallest at which each mechanism can
break: one vector per row, exactly one sweep of the workgroup, one sweep
plus a vector, the bench vocab, an odd vocab (unaligned rows, scalar
head and tail), and fp32.  All tests require an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box
from realhf_amd.ops import functional as F  # noqa: E402
from realhf_amd.parallel import tp as tp_mod  # noqa: E402
from tests.test_fused_logprob import (  # noqa: E402
    NEG_INF,
    assert_logp_close,
    hand_combine,
    make_case,
)

BF16, FP32 = torch.bfloat16, torch.float32
# (n, V, dtype, with -inf rows)
CASES = [
    (5, 8, BF16, False),
    (3, 2048, BF16, False),
    (4, 2056, BF16, False),
    (3, 32000, BF16, False),
    (2, 50257, BF16, False),
    (2, 1028, FP32, False),
    (3, 2048, BF16, True),
    (4, 2056, BF16, True),
]
_cache = {}


def case(n, V, dtype, with_inf):
    """(logits on the GPU in `dtype`, labels, grad_out, oracle logp, oracle
    dlogits), computed once per shape and never modified."""
    key = (n, V, dtype, with_inf)
    if key not in _cache:
        x, labels = make_case(V, dtype == BF16, seed=1,
                              n_plain=n - 3 if with_inf else n)
        if not with_inf:
            x, labels = x[:n], labels[:n]
        assert x.shape == (n, V) and torch.isinf(x).any() == with_inf
        g = torch.Generator().manual_seed(7)
        go = torch.randn(n, generator=g).cuda()
        x, labels = x.cuda(), labels.cuda()
        x32 = x.clone().requires_grad_(True)
        want = torch.log_softmax(x32, -1).gather(
            1, labels.unsqueeze(1)).squeeze(1)
        (want_grad,) = torch.autograd.grad(want, x32, go)
        _cache[key] = (x.to(dtype), labels, go, want.detach(), want_grad)
    return _cache[key]


@pytest.mark.parametrize("n,V,dtype,with_inf", CASES)
def test_forward(n, V, dtype, with_inf):
    x, labels, _, want, _ = case(n, V, dtype, with_inf)
    stats = C.vocab_logprob_fwd(x, labels, 0, -100)
    assert all(s.dtype == FP32 and s.shape == (n,) for s in stats)
    assert not any(torch.isnan(s).any() for s in stats)
    # oracle: the torch statistics + combine in fp32 on the same values
    oracle, oracle_lse = F.combine_vocab_stats(
        *F.vocab_logprob_stats_ref(x.float(), labels))
    logp, lse = F.combine_vocab_stats(*stats)
    fin = ~torch.isinf(oracle)
    print("max |logp - oracle|",
          float((logp[fin] - oracle[fin]).abs().max()) if fin.any() else 0.0)
    assert_logp_close(logp, oracle)
    assert_logp_close(logp, want)
    torch.testing.assert_close(lse, oracle_lse, atol=1e-4, rtol=1e-4)
    assert torch.equal(stats[1], x.float().max(-1).values)  # rowmax is exact
    if with_inf:
        assert logp[-1] == NEG_INF  # the label whose own logit is -inf
    # the public op is the same numbers
    assert torch.equal(F.vocab_logprobs(x, labels), logp)


@pytest.mark.parametrize("n,V,dtype,with_inf", CASES)
def test_backward(n, V, dtype, with_inf):
    x, labels, go, _, want_grad = case(n, V, dtype, with_inf)
    xg = x.clone().requires_grad_(True)
    logp = F.vocab_logprobs(xg, labels)
    (got,) = torch.autograd.grad(logp, xg, go)
    assert got.dtype == dtype and got.shape == (n, V)
    assert not torch.isnan(got).any() and not torch.isinf(got).any()
    err = (got.float() - want_grad).abs()
    print("max abs err", float(err.max()), "max rel err",
          float((err / want_grad.abs().clamp(min=1e-30)).max()))
    if dtype == BF16:
        # the same fp32 quantity rounded once to bf16: two bf16 ulps
        torch.testing.assert_close(got.float(), want_grad,
                                   rtol=2 ** -7, atol=1e-8)
    else:
        torch.testing.assert_close(got, want_grad, rtol=1e-4, atol=1e-7)


def test_misaligned_view():
    """A contiguous view whose base is not 16-byte aligned: the forward
    peels a scalar head, the backward (whose output is aligned) goes
    scalar for the whole row."""
    V = 2049
    big, labels = make_case(V, True, seed=2, n_plain=4)
    x = big.cuda().to(BF16)[1:]
    labels = labels.cuda()[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    aligned = x.clone()
    assert aligned.data_ptr() % 16 == 0
    go = torch.randn(x.shape[0], device="cuda")
    outs = []
    for t in (x, aligned):
        tg = t.detach().requires_grad_(True)
        logp = F.vocab_logprobs(tg, labels)
        outs.append((logp.detach(), torch.autograd.grad(logp, tg, go)[0]))
    # (max, sum) merge order differs between the two splits of a row
    assert_logp_close(outs[0][0], outs[1][0], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(outs[0][1].float(), outs[1][1].float(),
                               rtol=2 ** -7, atol=1e-8)


def test_ignored_rows():
    n, V = 6, 2056
    x, labels, go, want, _ = case(4, V, BF16, False)
    g = torch.Generator().manual_seed(5)
    x = torch.cat([x, torch.randn(2, V, generator=g).cuda().to(BF16)])
    labels = torch.cat([labels, labels[:2]])
    ign = torch.tensor([True, False, False, True, False, True], device="cuda")
    labels = labels.masked_fill(ign, -100)
    # ignored rows are skipped unread: NaN logits there must not surface
    x[ign] = float("nan")
    t, m, s = C.vocab_logprob_fwd(x, labels, 0, -100)
    assert torch.equal(t[ign], torch.zeros(3, device="cuda"))
    assert torch.equal(m[ign], torch.zeros(3, device="cuda"))
    assert torch.equal(s[ign], torch.ones(3, device="cuda"))
    xg = x.clone().requires_grad_(True)
    logp = F.vocab_logprobs(xg, labels)
    assert torch.equal(logp[ign], torch.zeros(3, device="cuda"))
    assert_logp_close(logp[1:3], want[1:3])
    (dl,) = torch.autograd.grad(logp, xg, torch.randn(n, device="cuda"))
    assert torch.equal(dl[ign], torch.zeros(3, V, dtype=BF16, device="cuda"))
    assert not torch.isnan(dl).any() and (dl[~ign] != 0).any()


def test_labels_outside_local_slice():
    V = 2048
    torch.manual_seed(9)
    full = (torch.randn(4, 2 * V, device="cuda") * 8).to(BF16)
    hi = full[:, V:].contiguous()
    # below, inside (first and last column), above the slice [2048, 4096)
    labels = torch.tensor([5, 2048, 4095, 5000], device="cuda")
    outside = torch.tensor([True, False, False, True], device="cuda")
    t, m, s = C.vocab_logprob_fwd(hi, labels, V, -100)
    assert torch.equal(t[outside], torch.zeros(2, device="cuda"))
    assert torch.equal(t[~outside], torch.stack([hi[1, 0], hi[2, V - 1]]).float())
    lse = torch.logsumexp(full.float(), -1)
    go = torch.ones(4, device="cuda")
    dl = C.vocab_logprob_bwd(hi, labels, lse, go, V, -100).float()
    # grad_out = 1: every entry is -softmax <= 0 except a +1 at the label
    assert (dl[outside] <= 0).all()
    pos = dl[~outside] > 0
    assert torch.equal(pos.sum(-1), torch.ones(2, dtype=torch.long, device="cuda"))
    assert pos[0, 0] and pos[1, V - 1]
    torch.testing.assert_close(
        dl, F.vocab_logprob_bwd_ref(hi, labels, lse, go, V).float(),
        rtol=2 ** -7, atol=1e-8)

    # two slices of the (4, 4096) problem combined on the one GPU
    labels = torch.tensor([5, 2048, 4095, 3000], device="cuda")
    lo = full[:, :V].contiguous()
    parts = [C.vocab_logprob_fwd(lo, labels, 0, -100),
             C.vocab_logprob_fwd(hi, labels, V, -100)]
    logp, _ = hand_combine(parts)
    whole, _ = F.combine_vocab_stats(*C.vocab_logprob_fwd(full, labels, 0, -100))
    torch.testing.assert_close(logp, whole, atol=1e-5, rtol=1e-5)
    want = torch.log_softmax(full.float(), -1).gather(
        1, labels.unsqueeze(1)).squeeze(1)
    torch.testing.assert_close(logp, want, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("n,V,dtype,with_inf",
                         [(4, 2056, BF16, True), (2, 50257, BF16, False)])
def test_run_to_run(n, V, dtype, with_inf):
    x, labels, go, _, _ = case(n, V, dtype, with_inf)
    a = C.vocab_logprob_fwd(x, labels, 0, -100)
    b = C.vocab_logprob_fwd(x, labels, 0, -100)
    # bitwise, -inf included (torch.equal treats equal infinities as equal)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    _, lse = F.combine_vocab_stats(*a)
    da = C.vocab_logprob_bwd(x, labels, lse, go, 0, -100)
    db = C.vocab_logprob_bwd(x, labels, lse, go, 0, -100)
    assert torch.equal(da, db)


def _peaks(x, cu, ids):
    """Peak allocation above the pre-call level of one
    packed_shifted_logprobs forward and of its backward."""
    xg = x.detach().requires_grad_(True)
    go = torch.randn(x.shape[0] - (cu.shape[0] - 1), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    logp = tp_mod.packed_shifted_logprobs(xg, cu, ids)
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (g,) = torch.autograd.grad(logp, xg, go)
    torch.cuda.synchronize()
    bwd = torch.cuda.max_memory_allocated() - base
    return fwd, bwd


def test_memory(monkeypatch):
    """Derived from the design, not measured: the fused forward allocates
    no [n, V]-sized tensor of any dtype, the fused backward only its
    output; the existing path holds three fp32 [n', V] tensors."""
    n, V = 256, 32000
    torch.manual_seed(4)
    x = torch.randn(n, V, device="cuda").to(BF16)
    ids = torch.randint(0, V, (n,), device="cuda")
    cu = torch.tensor([0, 128, 256], dtype=torch.int32, device="cuda")
    monkeypatch.setenv("REALHF_AMD_FUSED_LOGPROB", "1")
    fwd, bwd = _peaks(x, cu, ids)
    print("fused peaks", fwd, bwd, "n*V*2 =", n * V * 2)
    assert fwd < n * V * 2
    assert bwd < 2 * n * V * 2
    monkeypatch.delenv("REALHF_AMD_FUSED_LOGPROB")
    fwd_off, _ = _peaks(x, cu, ids)
    print("torch-path forward peak", fwd_off)
    assert fwd_off > 3 * n * V * 4  # the probe can see the difference


def _sft_step():
    import realhf_amd.interfaces  # noqa: F401
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.api.config import Abstraction, ModelName
    from realhf_amd.api.data import SequenceSample
    from realhf_amd.api.model import (
        FinetuneSpec,
        Model,
        make_backend,
        make_interface,
    )
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=2, hidden_dim=1024, n_heads=8, n_kv_heads=8, vocab_size=512,
        head_dim=128, intermediate_dim=2816, max_position_embeddings=2048,
    )
    cfg.family = "llama"
    m = ReaLModel(cfg, device="cuda:0", dtype=BF16)
    torch.manual_seed(0)
    m.random_init()
    model = Model(name=ModelName("actor", 0), module=m, tokenizer=None,
                  device=torch.device("cuda:0"), dtype=BF16)
    backend = make_backend(Abstraction("zero1", {"optimizer": {"lr": 1e-4}}))
    model = backend.initialize(model, FinetuneSpec(1, 64, 8))
    rng = np.random.RandomState(0)
    samples = []
    for i in range(4):
        l = int(rng.randint(32, 64))
        toks = torch.from_numpy(rng.randint(0, cfg.vocab_size, size=l)).long().cuda()
        pm = torch.zeros(l, dtype=torch.bool).cuda()
        pm[: l // 2] = True
        samples.append(SequenceSample(
            keys=("packed_input_ids", "prompt_mask"), ids=[f"s{i}"],
            seqlens={"packed_input_ids": [[l]], "prompt_mask": [[l]]},
            data={"packed_input_ids": toks, "prompt_mask": pm},
        ))
    batch = SequenceSample.gather(samples)
    return make_interface(Abstraction("sft")).train_step(model, batch)


def test_sft_step_flag_on_matches_off(monkeypatch):
    monkeypatch.delenv("REALHF_AMD_FUSED_LOGPROB", raising=False)
    off = _sft_step()
    calls = []
    real = C.vocab_logprob_bwd
    monkeypatch.setattr(C, "vocab_logprob_bwd",
                        lambda *a: calls.append(1) or real(*a))
    monkeypatch.setenv("REALHF_AMD_FUSED_LOGPROB", "1")
    on = _sft_step()
    assert calls  # the HIP backward ran inside the train step
    print("loss off/on", off["loss"], on["loss"])
    assert all(v == v for v in on.values()), on  # no NaN
    assert all(v == v for v in off.values()), off
    assert on["loss"] == pytest.approx(off["loss"], rel=1e-3)
