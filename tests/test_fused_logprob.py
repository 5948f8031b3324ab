"""Fused vocab log-prob op (ops.functional.vocab_logprobs), CPU side: the
torch statistics + combine formulation against log_softmax/gather, the
two-slice combine, the REALHF_AMD_FUSED_LOGPROB wiring in parallel/tp.py
and one two-rank TP case."""
import os

import numpy as np
import pytest
import torch

from realhf_amd.ops import functional as F

NEG_INF = float("-inf")
VOCABS = [1, 7, 8, 2048, 2056, 50257]


def make_case(V, bf16_valued, seed=0, n_plain=4, scale=8.0):
    """(logits fp32 [n, V], labels [n]).  After n_plain random rows come,
    for V >= 2, the three -inf rows: a leading all -inf chunk (the first
    min(2048, V - 1) columns), a single surviving column, and a label
    whose own logit is -inf."""
    g = torch.Generator().manual_seed(seed * 1000 + V)
    n = n_plain + (3 if V >= 2 else 0)
    x = torch.randn(n, V, generator=g) * scale
    if bf16_valued:
        x = x.bfloat16().float()
    labels = torch.randint(0, V, (n,), generator=g)
    if V >= 2:
        lead = min(2048, V - 1)
        x[n_plain, :lead] = NEG_INF
        labels[n_plain] = lead + int(labels[n_plain]) % (V - lead)
        keep = int(labels[n_plain + 1])
        row = torch.full((V,), NEG_INF)
        row[keep] = x[n_plain + 1, keep]
        x[n_plain + 1] = row
        x[n_plain + 2, int(labels[n_plain + 2])] = NEG_INF
    return x, labels


def reference_logp(x, labels):
    return torch.log_softmax(x.float(), -1).gather(
        1, labels.unsqueeze(1)).squeeze(1)


def assert_logp_close(got, want, atol=1e-4, rtol=1e-4):
    assert not torch.isnan(got).any()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf)
    assert torch.equal(got[inf], want[inf])  # same sign of infinity
    torch.testing.assert_close(got[~inf], want[~inf], atol=atol, rtol=rtol)


@pytest.mark.parametrize("bf16_valued", [False, True])
@pytest.mark.parametrize("V", VOCABS)
def test_single_rank_values(V, bf16_valued):
    x, labels = make_case(V, bf16_valued)
    want = reference_logp(x, labels)
    if V >= 2:
        assert want[-1] == NEG_INF  # the masked label
    logp, lse = F.combine_vocab_stats(*F.vocab_logprob_stats_ref(x, labels))
    assert_logp_close(logp, want)
    torch.testing.assert_close(lse, torch.logsumexp(x, -1),
                               atol=1e-4, rtol=1e-4)
    # the public op: ignored rows give 0, the others are unchanged
    ign = torch.arange(x.shape[0]) % 3 == 1
    got = F.vocab_logprobs(x, labels.masked_fill(ign, -100))
    assert got.dtype == torch.float32
    assert torch.equal(got[ign], torch.zeros(int(ign.sum())))
    assert_logp_close(got[~ign], want[~ign])


def test_ignored_rows_stats():
    x, labels = make_case(8, False)
    labels[1] = -100
    t, m, s = F.vocab_logprob_stats_ref(x, labels)
    assert (t[1], m[1], s[1]) == (0.0, 0.0, 1.0)


def hand_combine(stats):
    """Merge per-slice (target, rowmax, sumexp) without a process group."""
    t = torch.stack([s[0] for s in stats])
    m = torch.stack([s[1] for s in stats])
    se = torch.stack([s[2] for s in stats])
    g = m.max(0).values
    f = torch.where(se == 0, torch.zeros_like(se), (m - g).exp())
    lse = g + (se * f).sum(0).log()
    return t.sum(0) - lse, lse


@pytest.mark.parametrize("bf16_valued", [False, True])
@pytest.mark.parametrize("V", [v for v in VOCABS if v >= 2])
def test_two_slice_combine(V, bf16_valued):
    x, labels = make_case(V, bf16_valued)
    h = V // 2
    stats = [
        F.vocab_logprob_stats_ref(x[:, :h], labels, vocab_start=0),
        F.vocab_logprob_stats_ref(x[:, h:], labels, vocab_start=h),
    ]
    # a label lives in exactly one slice; the other reports target 0
    in_lo = labels < h
    assert torch.equal(stats[1][0][in_lo], torch.zeros(int(in_lo.sum())))
    assert torch.equal(stats[0][0][~in_lo], torch.zeros(int((~in_lo).sum())))
    # the single-survivor row leaves one slice entirely -inf
    assert any((s[1] == NEG_INF).any() and (s[2] == 0).any() for s in stats)
    logp, lse = hand_combine(stats)
    full, full_lse = F.combine_vocab_stats(*F.vocab_logprob_stats_ref(x, labels))
    assert_logp_close(logp, full, atol=1e-5, rtol=1e-5)
    assert_logp_close(logp, reference_logp(x, labels))
    torch.testing.assert_close(lse, full_lse, atol=1e-5, rtol=1e-5)


def _packed_case(lens, V, seed=3):
    g = torch.Generator().manual_seed(seed)
    total = sum(lens)
    logits = torch.randn(total, V, generator=g) * 4
    ids = torch.randint(0, V, (total,), generator=g)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    w = torch.randn(total - len(lens), generator=g)
    return logits, ids, cu, w


def _run_packed(logits, ids, cu, w):
    from realhf_amd.parallel.tp import packed_shifted_logprobs

    x = logits.clone().requires_grad_(True)
    lp = packed_shifted_logprobs(x, cu, ids)
    (lp * w).sum().backward()
    return lp.detach(), x.grad


def test_flag_on_matches_flag_off(monkeypatch):
    lens = [1, 2, 17, 64]  # the length-1 sequence has no predicting row
    logits, ids, cu, w = _packed_case(lens, V=50)
    monkeypatch.delenv("REALHF_AMD_FUSED_LOGPROB", raising=False)
    lp_off, g_off = _run_packed(logits, ids, cu, w)

    calls = []
    real = F.vocab_logprobs
    monkeypatch.setattr(
        F, "vocab_logprobs",
        lambda *a, **k: calls.append(a[0].shape) or real(*a, **k))
    monkeypatch.setenv("REALHF_AMD_FUSED_LOGPROB", "1")
    lp_on, g_on = _run_packed(logits, ids, cu, w)
    # the op ran over all `total` rows, not over a logits[leave] copy
    assert calls == [logits.shape]
    assert lp_on.shape == (sum(lens) - len(lens),)
    torch.testing.assert_close(lp_on, lp_off, atol=1e-5, rtol=0)
    torch.testing.assert_close(g_on, g_off, atol=1e-5, rtol=0)
    ends = cu[1:].long() - 1
    assert torch.equal(g_on[ends], torch.zeros(len(lens), logits.shape[1]))


def test_flag_keeps_fp16_on_existing_path(monkeypatch):
    monkeypatch.setenv("REALHF_AMD_FUSED_LOGPROB", "1")
    monkeypatch.setattr(F, "vocab_logprobs", None)  # would raise if called
    from realhf_amd.parallel.tp import packed_shifted_logprobs

    logits, ids, cu, _ = _packed_case([3, 4], V=16)
    lp = packed_shifted_logprobs(logits.half(), cu, ids)
    assert lp.shape == (5,)


def _tp2_fused_worker():
    """Masked + temperature-scaled log-probs and their gradient under TP
    vocab sharding with the fused path on, against the single-process
    reference (pattern of test_logits_mask._tp2_masked_logprob_worker)."""
    import torch.distributed as dist

    from realhf_amd.api.data import SequenceSample
    from realhf_amd.base import constants
    from realhf_amd.base.testing import init_global_constants
    from realhf_amd.interfaces.ppo import _warp_logits_like_sampler
    from realhf_amd.models.hf.llama import make_test_config
    from realhf_amd.models.real_model import ReaLModel
    from realhf_amd.parallel import tp as tp_mod
    from realhf_amd.utils.functional import build_shift_one_indices
    from tests.test_realloc import _fill_model_from_full, _full_reference_sd

    os.environ["REALHF_AMD_FUSED_LOGPROB"] = "1"
    cfg = make_test_config(n_layers=2, hidden_dim=64, n_heads=8, n_kv_heads=4,
                           vocab_size=128)
    cfg.dtype = "float32"
    sd = _full_reference_sd(cfg, seed=57)
    init_global_constants(num_dp=1, num_tp=2, num_pp=1, model_name="m")
    g = constants.grid_of("m")

    rng = np.random.RandomState(6)
    toks = torch.from_numpy(rng.randint(0, 128, size=18)).long()
    cu = torch.tensor([0, 10, 18], dtype=torch.int32)
    torch.manual_seed(11)  # same mask and weights on both ranks
    lm = torch.rand(16, 128) > 0.4
    w = torch.randn(16)
    nxt = toks[build_shift_one_indices(18, cu)]
    lm[torch.arange(16), nxt] = False
    mb = SequenceSample(
        keys=("packed_input_ids", "packed_logits_mask"),
        ids=["a", "b"],
        seqlens={"packed_input_ids": [[10], [8]],
                 "packed_logits_mask": [[9], [7]]},
        data={"packed_input_ids": toks, "packed_logits_mask": lm},
    )

    with constants.model_scope("m"):
        m = ReaLModel(cfg, device="cpu", dtype=torch.float32,
                      tp_rank=g.tp_rank, tp_size=2)
        _fill_model_from_full(m, cfg, sd)
        with torch.no_grad():
            logits = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=10)
            _warp_logits_like_sampler(logits, cu, mb, temperature=0.7)
        logits = logits.detach().requires_grad_(True)
        assert logits.shape == (18, 64) and tp_mod._use_fused(logits)
        lp = tp_mod.packed_shifted_logprobs(logits, cu, toks)
        (lp * w).sum().backward()
    tp_rank = g.tp_rank

    single = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    _fill_model_from_full(single, cfg, sd)
    constants.clear_grids()
    with torch.no_grad():
        full = single(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=10)
        full = full / 0.7
        rows = torch.arange(18)[~torch.isin(
            torch.arange(18), cu[1:].long() - 1)]  # leave-one rows
        full[rows] = full[rows].masked_fill(lm, NEG_INF)
    full.requires_grad_(True)
    want = torch.log_softmax(full.float(), -1)
    want = want[rows].gather(1, nxt.unsqueeze(1)).squeeze(1)
    (want * w).sum().backward()
    torch.testing.assert_close(lp.detach(), want.detach(), atol=1e-4, rtol=1e-4)
    want_grad = full.grad[:, tp_rank * 64:(tp_rank + 1) * 64]
    assert not torch.isnan(logits.grad).any()
    torch.testing.assert_close(logits.grad, want_grad, atol=1e-5, rtol=1e-4)
    dist.barrier()


@pytest.mark.distributed
def test_tp2_fused_logprobs_match_single():
    from realhf_amd.base.testing import LocalMultiProcessTest

    LocalMultiProcessTest(2, _tp2_fused_worker, backend="gloo").launch()
