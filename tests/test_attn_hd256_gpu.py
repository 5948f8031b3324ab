"""head_dim 256 (gemma) on the HIP attention path: the varlen forward and
MFMA backward, single-token decode, the fused decode epilogue, the Python
dispatch, hipGraph generation and one train step.  Kernel outputs are
compared with the fp32 CPU references at the tolerances the same tests use
at head_dim 128 with the same input scaling: head_dim enters only the QK^T
sum (exact bf16 products, fp32 accumulation), P and dS are rounded to bf16
exactly as at 128, and the output is a convex combination of V rows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

HD = 256
SCALE = 1.0 / np.sqrt(HD)


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32,
                        device="cuda")


def _qkv(lens, nq, nkv, mag, seed):
    torch.manual_seed(seed)
    total = sum(lens)
    return tuple(
        (torch.randn(total, n, HD, device="cuda") * mag).to(torch.bfloat16)
        for n in (nq, nkv, nkv))


# ---------------------------------------------------------------------------
# varlen forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1)])
def test_attn_varlen_fwd_hd256(nq, nkv, causal):
    """L = 1, a sequence inside one tile, and three query blocks with six KV
    tiles whose last tile has 10 keys."""
    lens = [1, 17, 330]
    q, k, v = _qkv(lens, nq, nkv, 0.5, 6)
    cu = _cu(lens)
    out, lse = C.attn_varlen_fwd(q, k, v, cu, max(lens), causal, SCALE, 0)
    qf, kf, vf = q.float().cpu(), k.float().cpu(), v.float().cpu()
    ref = F.attn_varlen_ref(qf, kf, vf, cu.cpu(), causal, SCALE)
    err = (out.float().cpu() - ref).abs().max().item()
    print("fwd hd256", (nq, nkv), "causal", causal, "max |out - ref|", err)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)
    assert torch.isfinite(lse).all()
    if causal:
        # row 0 of a sequence sees key 0 only: lse = that one score
        rep = nq // nkv
        for s in cu[:-1].tolist():
            score = (qf[s] * kf[s].repeat_interleave(rep, dim=0)).sum(-1) * SCALE
            lerr = (lse[s].cpu() - score).abs().max().item()
            print("  seq start", s, "max |lse - ref|", lerr)
            assert lerr <= 1e-2, (s, lerr)


def test_attn_varlen_fwd_hd256_sliding_window():
    """Window 48 over [130, 64]: kv_begin > 0 in the second query block."""
    lens, window = [130, 64], 48
    q, k, v = _qkv(lens, 4, 4, 0.5, 31)
    cu = _cu(lens)
    out, _ = C.attn_varlen_fwd(q, k, v, cu, max(lens), True, SCALE, window)
    ref = F.attn_varlen_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(),
                            cu.cpu(), True, SCALE, window=window)
    err = (out.float().cpu() - ref).abs().max().item()
    print("fwd hd256 window", window, "max |out - ref|", err)
    torch.testing.assert_close(out.float().cpu(), ref, atol=0.05, rtol=3e-2)
    full, _ = C.attn_varlen_fwd(q, k, v, cu, max(lens), True, SCALE, 0)
    assert not torch.allclose(out, full)


# ---------------------------------------------------------------------------
# varlen backward
# ---------------------------------------------------------------------------
def _bwd_case(nq, nkv, window):
    lens = [96, 64, 130, 32]
    total = sum(lens)
    q, k, v = _qkv(lens, nq, nkv, 0.3, 21)
    dout = (torch.randn(total, nq, HD, device="cuda") * 0.3).to(torch.bfloat16)
    cu = _cu(lens)
    # fp32 reference grads: autograd over the blocked torch implementation
    # (on the CPU every matmul of it is fp32)
    qr, kr, vr = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
    ref = F._attn_varlen_blocked_torch(qr, kr, vr, cu.cpu(), True, SCALE,
                                       window=window or None)
    refs = torch.autograd.grad(ref, (qr, kr, vr), dout.float().cpu())
    out, lse = C.attn_varlen_fwd(q, k, v, cu, max(lens), True, SCALE, window)
    dsum = (dout.float() * out.float()).sum(-1)
    args = (q, k, v, dout, lse, dsum, cu, True, SCALE, window)

    def check(tag, dq32, dk32, dv32):
        rep = nq // nkv
        if rep > 1:
            dk32 = dk32.view(total, nkv, rep, HD).sum(2)
            dv32 = dv32.view(total, nkv, rep, HD).sum(2)
        for name, got, want in zip(("dq", "dk", "dv"), (dq32, dk32, dv32), refs):
            err = (got.cpu() - want).abs().max().item()
            print("bwd hd256", (nq, nkv), "window", window, tag, name,
                  "max err", err)
            torch.testing.assert_close(got.cpu(), want, atol=0.15, rtol=5e-2)

    return args, check


@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1)])
def test_attn_varlen_bwd_hd256(nq, nkv):
    """Atomic dQ, deterministic dQ (bit-identical from call to call), and a
    max_seqlen that is too small: the order is lost, no contribution is."""
    args, check = _bwd_case(nq, nkv, 0)
    atomic = C.attn_varlen_bwd(*args, 0)
    check("atomic", *atomic)
    det1 = C.attn_varlen_bwd(*args, 130)
    det2 = C.attn_varlen_bwd(*args, 130)
    check("det", *det1)
    assert torch.equal(det1[0], det2[0])
    assert torch.equal(det1[1], atomic[1]) and torch.equal(det1[2], atomic[2])
    short = C.attn_varlen_bwd(*args, 64)
    check("det max_seqlen=64", *short)
    # the same fp32 partials in another order: at most 3 terms per element
    torch.testing.assert_close(short[0], atomic[0], atol=1e-5, rtol=1e-5)


def test_attn_varlen_bwd_hd256_sliding_window():
    args, check = _bwd_case(4, 4, 48)
    got = C.attn_varlen_bwd(*args, 0)
    check("atomic", *got)
    check("det", *C.attn_varlen_bwd(*args, 130))
    full = C.attn_varlen_bwd(*args[:-1], 0, 0)
    assert not torch.allclose(got[0], full[0])


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
_DEC_LENS = [1, 50, 200, 399, 64]


def _decode_case(nq, nkv, window=0, seed=7):
    torch.manual_seed(seed)
    bs, maxlen = 5, 400
    lens = torch.tensor(_DEC_LENS, dtype=torch.int32, device="cuda")
    q = torch.randn(bs, nq, HD, dtype=torch.bfloat16, device="cuda") * 0.5
    kc = torch.randn(bs, maxlen, nkv, HD, dtype=torch.bfloat16, device="cuda") * 0.5
    vc = torch.randn(bs, maxlen, nkv, HD, dtype=torch.bfloat16, device="cuda") * 0.5
    ref = F.attn_decode_ref(q.float().cpu(), kc.float().cpu(), vc.float().cpu(),
                            lens.cpu(), SCALE, window=window or None)
    return q, kc, vc, lens, ref


@pytest.mark.parametrize("nq,nkv", [(16, 16), (8, 1), (8, 4), (8, 2)])
def test_attn_decode_hd256(nq, nkv):
    q, kc, vc, lens, ref = _decode_case(nq, nkv)
    out = C.attn_decode(q, kc, vc, lens, SCALE, 0)
    err = (out.float().cpu() - ref).abs().max().item()
    print("decode hd256 rep", nq // nkv, "max |out - ref|", err)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


def test_attn_decode_hd256_sliding_window():
    q, kc, vc, lens, ref = _decode_case(8, 4, window=48)
    out = C.attn_decode(q, kc, vc, lens, SCALE, 48)
    err = (out.float().cpu() - ref).abs().max().item()
    print("decode hd256 window 48 max |out - ref|", err)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)
    assert not torch.allclose(out, C.attn_decode(q, kc, vc, lens, SCALE, 0))


# Runs in a fresh interpreter: the extension reads REALHF_AMD_DEC_WAVES and
# REALHF_AMD_DEC_SPLIT once per process.
_DEC_CHILD = r"""
import faulthandler
faulthandler.dump_traceback_later(100, exit=True)
import numpy as np
import torch
from realhf_amd.ops import functional as F
import realhf_amd._C as C

hd, bs, maxlen = 256, 5, 400
scale = 1.0 / np.sqrt(hd)
for nq, nkv in ((16, 16), (8, 1)):
    torch.manual_seed(7)
    lens = torch.tensor([1, 50, 200, 399, 64], dtype=torch.int32, device="cuda")
    q = torch.randn(bs, nq, hd, dtype=torch.bfloat16, device="cuda") * 0.5
    kc = torch.randn(bs, maxlen, nkv, hd, dtype=torch.bfloat16, device="cuda") * 0.5
    vc = torch.randn(bs, maxlen, nkv, hd, dtype=torch.bfloat16, device="cuda") * 0.5
    out = C.attn_decode(q, kc, vc, lens, scale, 0)
    ref = F.attn_decode_ref(q.float().cpu(), kc.float().cpu(), vc.float().cpu(),
                            lens.cpu(), scale)
    err = (out.float().cpu() - ref).abs().max().item()
    print("rep", nq // nkv, "max |out - ref|", err, flush=True)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)
"""


@pytest.mark.parametrize("env", [
    {"REALHF_AMD_DEC_WAVES": "2"},
    {"REALHF_AMD_DEC_WAVES": "4"},
    {"REALHF_AMD_DEC_WAVES": "8"},  # does not fit LDS at 256: runs with 4
    {"REALHF_AMD_DEC_SPLIT": "1"},  # one split: the no-workspace path
], ids=lambda e: "-".join(f"{k[11:]}{v}" for k, v in e.items()))
def test_attn_decode_hd256_env_variants(env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    base = {k: v for k, v in os.environ.items()
            if k not in ("REALHF_AMD_DEC_WAVES", "REALHF_AMD_DEC_SPLIT")}
    r = subprocess.run(
        cmd + ["-c", _DEC_CHILD], cwd=root, timeout=120,
        env=dict(base, **env), capture_output=True, text=True,
    )
    print(r.stdout)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"


# ---------------------------------------------------------------------------
# Python dispatch
# ---------------------------------------------------------------------------
def test_attn_varlen_dispatch_hd256():
    """F.attn_varlen at 256 is the HIP autograd function (forward + MFMA
    backward), not the padded torch path."""
    torch.manual_seed(8)
    lens = [96, 130]
    nq = nkv = 4
    q, k, v = _qkv(lens, nq, nkv, 0.5, 8)
    cu = _cu(lens)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = F.attn_varlen(qg, kg, vg, cu, max(lens), True, None)
    assert type(out.grad_fn).__name__.startswith("_AttnVarlenFn"), out.grad_fn
    g = torch.randn_like(out)
    out.backward(g)
    qr, kr, vr = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
    ref = F.attn_varlen_ref(qr, kr, vr, cu.cpu(), True, SCALE)
    ref.backward(g.float().cpu())
    torch.testing.assert_close(out.float().cpu(), ref, atol=4e-2, rtol=4e-2)
    for name, got, want in (("dq", qg, qr), ("dk", kg, kr), ("dv", vg, vr)):
        err = (got.grad.float().cpu() - want.grad).abs().max().item()
        print("dispatch hd256", name, "max err", err)
        torch.testing.assert_close(got.grad.float().cpu(), want.grad,
                                   atol=8e-2, rtol=8e-2)


def test_attn_decode_dispatch_hd256(monkeypatch):
    q, kc, vc, lens, ref = _decode_case(8, 1)

    def boom(*a, **kw):
        raise AssertionError("attn_decode_ref called at head_dim 256")

    monkeypatch.setattr(F, "attn_decode_ref", boom)
    out = F.attn_decode(q, kc, vc, lens)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


# ---------------------------------------------------------------------------
# model level: fused decode epilogue, hipGraph generation, one train step
# ---------------------------------------------------------------------------
def _gemma_cfg(n_layers):
    import realhf_amd.models.hf as hf_reg

    cfg = hf_reg.get_family("gemma").make_test_config(
        n_layers=n_layers, hidden_dim=256, n_heads=2, n_kv_heads=1,
        head_dim=HD, vocab_size=256, intermediate_dim=512,
    )
    cfg.family = "gemma"
    return cfg


def test_fused_decode_layer_hd256_matches_eager(monkeypatch):
    """A gemma layer at 256 takes the fused rope_qkv_decode epilogue, and it
    agrees with the composed eager decode path: logits and appended K/V."""
    from realhf_amd.models.real_model import ReaLModel

    cfg = _gemma_cfg(1)
    torch.manual_seed(11)
    model = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    model.random_init()
    bs, maxlen = 3, 32
    kv = [(torch.zeros(bs, maxlen, 1, HD, dtype=torch.bfloat16, device="cuda"),
           torch.zeros(bs, maxlen, 1, HD, dtype=torch.bfloat16, device="cuda"))
          for _ in range(cfg.n_layers)]
    kv2 = [(k.clone(), v.clone()) for k, v in kv]
    tokens = torch.randint(0, 256, (bs,), device="cuda")
    cache_seqlens = torch.tensor([5, 9, 2], dtype=torch.int32, device="cuda")

    calls = []
    real = C.rope_qkv_decode

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(C, "rope_qkv_decode", spy)
    with torch.no_grad():
        out_fused = model(packed_input_ids=tokens, kv_caches=kv,
                          cache_seqlens=cache_seqlens, decode=True)
        assert len(calls) == cfg.n_layers  # the fused path ran
        monkeypatch.setenv("REALHF_AMD_NO_FUSED_DECODE", "1")
        out_eager = model(packed_input_ids=tokens, kv_caches=kv2,
                          cache_seqlens=cache_seqlens, decode=True)
        assert len(calls) == cfg.n_layers
    torch.testing.assert_close(out_fused.float(), out_eager.float(),
                               atol=3e-2, rtol=3e-2)
    for (k1, v1), (k2, v2) in zip(kv, kv2):
        assert k1.abs().sum() > 0
        torch.testing.assert_close(k1.float(), k2.float(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(v1.float(), v2.float(), atol=2e-2, rtol=2e-2)


def test_generate_hd256_captures_decode_graph(monkeypatch):
    """generate() at 256 captures the decode hipGraph, and the graph's tokens
    equal those of eager decode."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models.generation import generate
    from realhf_amd.models.real_model import ReaLModel

    cfg = _gemma_cfg(2)
    torch.manual_seed(44)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init()
    toks = torch.randint(0, 256, (24,), device="cuda")
    cu = torch.tensor([0, 12, 24], dtype=torch.int32, device="cuda")
    g = GenerationHyperparameters(max_new_tokens=8, greedy=True,
                                  use_hip_graph=True)
    out_graph = generate(m, toks, cu, g)
    assert m._gen_session[1].decoder.graph is not None
    m._gen_session = None  # fresh session for the failing-capture run
    monkeypatch.setenv("REALHF_AMD_FORCE_GRAPH_FAIL", "1")
    out_eager = generate(m, toks, cu, g)
    assert m._gen_session[1].decoder.graph is None
    assert torch.equal(out_graph.gen_tokens, out_eager.gen_tokens)


def test_sft_step_hd256():
    """One SFT train step (forward, MFMA backward, optimizer) on a gemma
    config at 256 returns finite stats."""
    import realhf_amd.interfaces  # noqa: F401
    from realhf_amd.api.config import Abstraction, ModelName
    from realhf_amd.api.data import SequenceSample
    from realhf_amd.api.model import (FinetuneSpec, Model, make_backend,
                                      make_interface)
    from realhf_amd.models.real_model import ReaLModel

    cfg = _gemma_cfg(2)
    m = ReaLModel(cfg, device="cuda:0", dtype=torch.bfloat16)
    torch.manual_seed(0)
    m.random_init()
    model = Model(name=ModelName("actor", 0), module=m, tokenizer=None,
                  device=torch.device("cuda:0"), dtype=torch.bfloat16)
    backend = make_backend(Abstraction("zero1", {"optimizer": {"lr": 1e-4}}))
    model = backend.initialize(model, FinetuneSpec(1, 64, 8))
    rng = np.random.RandomState(0)
    samples = []
    for i, l in enumerate((33, 64, 47, 70)):
        toks = torch.from_numpy(rng.randint(0, cfg.vocab_size, size=l)).long().cuda()
        pm = torch.zeros(l, dtype=torch.bool).cuda()
        pm[: l // 2] = True
        samples.append(SequenceSample(
            keys=("packed_input_ids", "prompt_mask"), ids=[f"s{i}"],
            seqlens={"packed_input_ids": [[l]], "prompt_mask": [[l]]},
            data={"packed_input_ids": toks, "prompt_mask": pm}))
    stats = make_interface(Abstraction("sft")).train_step(
        model, SequenceSample.gather(samples))
    assert stats and all(np.isfinite(v) for v in stats.values()), stats
