"""Gemma-2 on the HIP path: the attention logit soft-cap in the varlen
forward, the MFMA backward and decode attention (bf16 and FP8 caches), the
bindings' default argument, the Python dispatch, and a tiny gemma2 model
through the fused decode block, hipGraph generation, FP8 generation and one
train step.

Kernel outputs are compared with the fp32 CPU references (with `softcap`) at
the project's tolerances.  q and k are 1.5 * N(0, 1) so that a cap of 2.0
binds: the capped and uncapped references differ by far more than the
tolerance, and a kernel that ignores the argument cannot pass.  The tolerances
were set at smaller q / k, so every test first checks the uncapped kernel
against the uncapped reference on the same inputs (the control)."""
import copy
import functools
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

QK_MAG = 1.5
FWD_TOL = dict(atol=3e-2, rtol=3e-2)
BWD_TOL = dict(atol=0.15, rtol=5e-2)
CAPS = [2.0, 50.0]  # one that binds hard, and gemma-2's own


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32,
                        device="cuda")


def _scale(hd):
    return 1.0 / np.sqrt(hd)


def _maxerr(a, b):
    return (a - b).abs().max().item()


# ---------------------------------------------------------------------------
# varlen forward
# ---------------------------------------------------------------------------
FWD_LENS = [1, 17, 330]  # L = 1, inside one tile, a ragged last KV tile


@functools.lru_cache(maxsize=None)
def _fwd_case(hd, nq, nkv, lens, window):
    """Inputs (GPU, bf16) and the fp32 CPU references per cap (0 = no cap)."""
    torch.manual_seed(100 + hd + nq)
    total = sum(lens)
    q = (torch.randn(total, nq, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    k = (torch.randn(total, nkv, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    v = (torch.randn(total, nkv, hd, device="cuda") * 0.5).to(torch.bfloat16)
    cu = _cu(lens)
    qf, kf, vf = (t.float().cpu() for t in (q, k, v))
    refs = {cap: F.attn_varlen_ref(qf, kf, vf, cu.cpu(), True, _scale(hd),
                                   window=window, softcap=cap or None)
            for cap in [0.0] + CAPS}
    return q, k, v, cu, refs


def _fwd_check(hd, nq, nkv, lens, window, cap):
    q, k, v, cu, refs = _fwd_case(hd, nq, nkv, tuple(lens), window)
    scale, w = _scale(hd), int(window or 0)
    # control: the uncapped kernel on these inputs
    out0, _ = C.attn_varlen_fwd(q, k, v, cu, max(lens), True, scale, w)
    print(f"fwd hd{hd} {nq}/{nkv} window {w} control max err",
          _maxerr(out0.float().cpu(), refs[0.0]))
    torch.testing.assert_close(out0.float().cpu(), refs[0.0], **FWD_TOL)
    gap = _maxerr(refs[cap], refs[0.0])
    out, lse = C.attn_varlen_fwd(q, k, v, cu, max(lens), True, scale, w, cap)
    print(f"fwd hd{hd} {nq}/{nkv} window {w} softcap {cap} max err",
          _maxerr(out.float().cpu(), refs[cap]), "capped-vs-uncapped ref", gap)
    if cap == 2.0:  # the cap must bind: 10x atol at least
        assert gap >= 10 * FWD_TOL["atol"], gap
    torch.testing.assert_close(out.float().cpu(), refs[cap], **FWD_TOL)
    assert torch.isfinite(lse).all()
    return q, k, cu, lse


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_attn_varlen_fwd_softcap(hd, nq, nkv, cap):
    q, k, cu, lse = _fwd_check(hd, nq, nkv, FWD_LENS, None, cap)
    # row 0 of a sequence sees key 0 only: lse = that one capped score
    qf, kf = q.float().cpu(), k.float().cpu()
    for s in cu[:-1].tolist():
        x = (qf[s] * kf[s].repeat_interleave(nq // nkv, dim=0)).sum(-1) * _scale(hd)
        want = cap * torch.tanh(x / cap)
        lerr = _maxerr(lse[s].cpu(), want)
        print("  seq start", s, "max |lse - cap*tanh(score/cap)|", lerr)
        assert lerr <= 1e-2, (s, lerr)


def test_attn_varlen_fwd_softcap_sliding_window():
    """Window 48 over [130, 64]: kv_begin > 0 in the second query block."""
    q, k, cu, _ = _fwd_check(128, 4, 4, [130, 64], 48, 2.0)


# ---------------------------------------------------------------------------
# varlen backward
# ---------------------------------------------------------------------------
BWD_LENS = [96, 64, 130, 32]


@functools.lru_cache(maxsize=None)
def _bwd_case(hd, nq, nkv, window):
    torch.manual_seed(200 + hd + nq)
    total = sum(BWD_LENS)
    q = (torch.randn(total, nq, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    k = (torch.randn(total, nkv, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    v = (torch.randn(total, nkv, hd, device="cuda") * 0.3).to(torch.bfloat16)
    dout = (torch.randn(total, nq, hd, device="cuda") * 0.3).to(torch.bfloat16)
    cu = _cu(BWD_LENS)
    refs = {}
    for cap in [0.0] + CAPS:
        # fp32 reference grads: autograd over the blocked torch implementation
        # (on the CPU every matmul of it is fp32)
        qr, kr, vr = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
        ref = F._attn_varlen_blocked_torch(
            qr, kr, vr, cu.cpu(), True, _scale(hd), window=window,
            softcap=cap or None)
        refs[cap] = torch.autograd.grad(ref, (qr, kr, vr), dout.float().cpu())
    return q, k, v, dout, cu, refs


def _bwd_run(hd, nq, nkv, window, cap, max_seqlen):
    q, k, v, dout, cu, _ = _bwd_case(hd, nq, nkv, window)
    w = int(window or 0)
    out, lse = C.attn_varlen_fwd(q, k, v, cu, max(BWD_LENS), True, _scale(hd),
                                 w, cap)
    dsum = (dout.float() * out.float()).sum(-1)
    return C.attn_varlen_bwd(q, k, v, dout, lse, dsum, cu, True, _scale(hd), w,
                             max_seqlen, cap)


def _bwd_compare(tag, hd, nq, nkv, got, want):
    total, rep = sum(BWD_LENS), nq // nkv
    dq32, dk32, dv32 = got
    if rep > 1:
        dk32 = dk32.view(total, nkv, rep, hd).sum(2)
        dv32 = dv32.view(total, nkv, rep, hd).sum(2)
    for name, g, r in zip(("dq", "dk", "dv"), (dq32, dk32, dv32), want):
        print(f"bwd hd{hd} {nq}/{nkv} {tag} {name} max err",
              _maxerr(g.cpu(), r), "max |ref|", r.abs().max().item())
        torch.testing.assert_close(g.cpu(), r, **BWD_TOL)


def _bwd_check(hd, nq, nkv, window, cap):
    refs = _bwd_case(hd, nq, nkv, window)[-1]
    # control: the uncapped kernel on these inputs
    control = _bwd_run(hd, nq, nkv, window, 0.0, 0)
    _bwd_compare("control", hd, nq, nkv, control, refs[0.0])
    gap = _maxerr(refs[cap][0], refs[0.0][0])
    print(f"bwd hd{hd} softcap {cap}: capped-vs-uncapped ref dq", gap)
    if cap == 2.0:
        # the cap must bind: with these lengths and dout = 0.3 the dQ gap is
        # 3-5x atol, and what a kernel that ignores the argument returns (the
        # control) is outside the tolerance of the capped reference
        assert gap >= 2 * BWD_TOL["atol"], gap
        assert not torch.allclose(control[0].cpu(), refs[cap][0], **BWD_TOL)
    atomic = _bwd_run(hd, nq, nkv, window, cap, 0)
    _bwd_compare(f"softcap {cap} atomic", hd, nq, nkv, atomic, refs[cap])
    det1 = _bwd_run(hd, nq, nkv, window, cap, 130)
    det2 = _bwd_run(hd, nq, nkv, window, cap, 130)
    _bwd_compare(f"softcap {cap} det", hd, nq, nkv, det1, refs[cap])
    assert torch.equal(det1[0], det2[0])  # bit-identical from call to call
    assert torch.equal(det1[1], atomic[1]) and torch.equal(det1[2], atomic[2])


@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_attn_varlen_bwd_softcap(hd, nq, nkv):
    _bwd_check(hd, nq, nkv, None, 2.0)


def test_attn_varlen_bwd_softcap_50():
    _bwd_check(256, 4, 4, None, 50.0)


def test_attn_varlen_bwd_softcap_sliding_window():
    _bwd_check(128, 4, 4, 48, 2.0)


def test_attn_varlen_bwd_recompute_fallback_takes_softcap(monkeypatch):
    """REALHF_AMD_NO_HIP_ATTN_BWD=1: the torch recompute applies the cap."""
    hd, nq, nkv = 128, 4, 4
    q, k, v, dout, cu, refs = _bwd_case(hd, nq, nkv, None)
    monkeypatch.setenv("REALHF_AMD_NO_HIP_ATTN_BWD", "1")
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = F.attn_varlen(qg, kg, vg, cu, max(BWD_LENS), True, None, softcap=2.0)
    out.backward(dout)
    for name, g, r in zip(("dq", "dk", "dv"), (qg, kg, vg), refs[2.0]):
        print("recompute fallback", name, "max err",
              _maxerr(g.grad.float().cpu(), r))
        # bf16 GEMMs and bf16 gradients: the dispatch test's bound at 256
        torch.testing.assert_close(g.grad.float().cpu(), r, atol=8e-2, rtol=8e-2)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
DEC_LENS = [1, 50, 200, 399, 64]


@functools.lru_cache(maxsize=None)
def _decode_case(hd, nq, nkv, fp8, window):
    """q, the caches (bf16 tensors or F.Fp8KVCache of the same values) and
    the fp32 CPU references per cap.  The FP8 reference runs on the
    dequantized cache: the kernel's only other input."""
    torch.manual_seed(300 + hd + nq + nkv)
    bs, maxlen = len(DEC_LENS), 400
    lens = torch.tensor(DEC_LENS, dtype=torch.int32, device="cuda")
    q = (torch.randn(bs, nq, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    kc = (torch.randn(bs, maxlen, nkv, hd) * QK_MAG).to(torch.bfloat16)
    vc = (torch.randn(bs, maxlen, nkv, hd) * 0.5).to(torch.bfloat16)
    if fp8:
        def quant(x):
            q8, s = F.quantize_rows_e4m3_ref(x.reshape(-1, hd))
            return F.Fp8KVCache(
                q8.reshape(bs, maxlen, nkv, hd),
                s.reshape(bs, maxlen, nkv).transpose(1, 2).contiguous())

        kq, vq = quant(kc), quant(vc)
        kf, vf = kq.dequantize(), vq.dequantize()
        kc, vc = (F.Fp8KVCache(c.codes.cuda(), c.scale.cuda()) for c in (kq, vq))
    else:
        kf, vf = kc.float(), vc.float()
        kc, vc = kc.cuda(), vc.cuda()
    refs = {cap: F.attn_decode_ref(q.float().cpu(), kf, vf, lens.cpu(),
                                   _scale(hd), window=window,
                                   softcap=cap or None)
            for cap in [0.0] + CAPS}
    return q, kc, vc, lens, refs


def _decode_call(q, kc, vc, lens, scale, window, *cap):
    if isinstance(kc, F.Fp8KVCache):
        return C.attn_decode_fp8(q, kc.codes, kc.scale, vc.codes, vc.scale,
                                 lens, scale, window, *cap)
    return C.attn_decode(q, kc, vc, lens, scale, window, *cap)


def _decode_check(hd, nq, nkv, fp8, window, cap):
    q, kc, vc, lens, refs = _decode_case(hd, nq, nkv, fp8, window)
    w, tag = int(window or 0), f"decode hd{hd} {nq}/{nkv} fp8 {fp8} window {window}"
    out0 = _decode_call(q, kc, vc, lens, _scale(hd), w)
    print(tag, "control max err", _maxerr(out0.float().cpu(), refs[0.0]))
    torch.testing.assert_close(out0.float().cpu(), refs[0.0], **FWD_TOL)
    gap = _maxerr(refs[cap], refs[0.0])
    out = _decode_call(q, kc, vc, lens, _scale(hd), w, cap)
    print(tag, "softcap", cap, "max err", _maxerr(out.float().cpu(), refs[cap]),
          "capped-vs-uncapped ref", gap)
    if cap == 2.0:
        assert gap >= 10 * FWD_TOL["atol"], gap
    torch.testing.assert_close(out.float().cpu(), refs[cap], **FWD_TOL)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("nq,nkv", [(8, 8), (8, 4), (8, 1)])
@pytest.mark.parametrize("hd", [128, 256])
def test_attn_decode_softcap(hd, nq, nkv, fp8, cap):
    _decode_check(hd, nq, nkv, fp8, None, cap)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_attn_decode_softcap_sliding_window(fp8):
    _decode_check(256, 8, 4, fp8, 48, 2.0)


# Runs in a fresh interpreter: the extension reads REALHF_AMD_DEC_SPLIT once
# per process.  One split is the no-workspace epilogue.
_DEC_CHILD = r"""
import faulthandler
faulthandler.dump_traceback_later(100, exit=True)
import numpy as np
import torch
from realhf_amd.ops import functional as F
import realhf_amd._C as C

bs, maxlen, cap = 5, 400, 2.0
for hd, nq, nkv in ((256, 8, 4), (128, 8, 1)):
    scale = 1.0 / np.sqrt(hd)
    torch.manual_seed(7)
    lens = torch.tensor([1, 50, 200, 399, 64], dtype=torch.int32, device="cuda")
    q = (torch.randn(bs, nq, hd, device="cuda") * 1.5).to(torch.bfloat16)
    kc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 1.5).to(torch.bfloat16)
    vc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 0.5).to(torch.bfloat16)
    out = C.attn_decode(q, kc, vc, lens, scale, 0, cap)
    ref = F.attn_decode_ref(q.float().cpu(), kc.float().cpu(), vc.float().cpu(),
                            lens.cpu(), scale, softcap=cap)
    err = (out.float().cpu() - ref).abs().max().item()
    print("hd", hd, "rep", nq // nkv, "max |out - ref|", err, flush=True)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)
"""


def test_attn_decode_softcap_one_split():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    r = subprocess.run(
        cmd + ["-c", _DEC_CHILD], cwd=root, timeout=120,
        env=dict(os.environ, REALHF_AMD_DEC_SPLIT="1"), capture_output=True,
        text=True,
    )
    print(r.stdout)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"


# ---------------------------------------------------------------------------
# saturation
# ---------------------------------------------------------------------------
def test_softcap_saturation():
    """q = k = 40 * ones on the first 16 rows at hd 128: score / softcap is in
    the thousands, tanh is exactly 1 and 1 - t^2 exactly 0.  Everything stays
    finite, and dQ of those rows, whose every visible key saturates, is 0."""
    hd, L, cap, nsat = 128, 96, 2.0, 16
    torch.manual_seed(5)
    q = (torch.randn(L, 1, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    k = (torch.randn(L, 1, hd, device="cuda") * QK_MAG).to(torch.bfloat16)
    v = (torch.randn(L, 1, hd, device="cuda") * 0.3).to(torch.bfloat16)
    dout = (torch.randn(L, 1, hd, device="cuda") * 0.3).to(torch.bfloat16)
    q[:nsat] = 40.0
    k[:nsat] = 40.0
    cu = _cu([L])
    out, lse = C.attn_varlen_fwd(q, k, v, cu, L, True, _scale(hd), 0, cap)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    ref = F.attn_varlen_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(),
                            cu.cpu(), True, _scale(hd), softcap=cap)
    torch.testing.assert_close(out.float().cpu(), ref, **FWD_TOL)
    dsum = (dout.float() * out.float()).sum(-1)
    for max_seqlen in (0, L):  # atomic and deterministic dQ
        dq, dk, dv = C.attn_varlen_bwd(q, k, v, dout, lse, dsum, cu, True,
                                       _scale(hd), 0, max_seqlen, cap)
        for g in (dq, dk, dv):
            assert torch.isfinite(g).all()
        assert (dq[:nsat] == 0).all(), dq[:nsat].abs().max()
        assert dq[nsat:].abs().max() > 0
    # decode over the same keys, the query saturating against the first 16
    kc, vc = k.view(1, L, 1, hd).contiguous(), v.view(1, L, 1, hd).contiguous()
    lens = torch.tensor([L], dtype=torch.int32, device="cuda")
    o = C.attn_decode(q[:1].contiguous(), kc, vc, lens, _scale(hd), 0, cap)
    assert torch.isfinite(o.float()).all()
    dref = F.attn_decode_ref(q[:1].float().cpu(), kc.float().cpu(),
                             vc.float().cpu(), lens.cpu(), _scale(hd),
                             softcap=cap)
    torch.testing.assert_close(o.float().cpu(), dref, **FWD_TOL)


# ---------------------------------------------------------------------------
# default argument and dispatch
# ---------------------------------------------------------------------------
def test_bindings_default_softcap(monkeypatch):
    """Without the argument, with 0.0, and through F.* with softcap=None: the
    same bits."""
    hd, nq, nkv = 128, 4, 4
    q, k, v, dout, cu, _ = _bwd_case(hd, nq, nkv, None)
    mx, scale = max(BWD_LENS), _scale(hd)
    out_a, lse_a = C.attn_varlen_fwd(q, k, v, cu, mx, True, scale, 0)
    out_b, lse_b = C.attn_varlen_fwd(q, k, v, cu, mx, True, scale, 0, 0.0)
    assert torch.equal(out_a, out_b) and torch.equal(lse_a, lse_b)
    dsum = (dout.float() * out_a.float()).sum(-1)
    args = (q, k, v, dout, lse_a, dsum, cu, True, scale, 0)
    g_a = C.attn_varlen_bwd(*args, mx)  # deterministic dQ: comparable bits
    g_b = C.attn_varlen_bwd(*args, mx, 0.0)
    g_c = C.attn_varlen_bwd(*args, max_seqlen=mx, softcap=0.0)
    for a, b, c in zip(g_a, g_b, g_c):
        assert torch.equal(a, b) and torch.equal(a, c)
    monkeypatch.setenv("REALHF_AMD_ATTN_BWD_DET", "1")
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out_f = F.attn_varlen(qg, kg, vg, cu, mx, True, None, softcap=None)
    assert torch.equal(out_f, out_a)
    out_f.backward(dout)
    for g, a in zip((qg, kg, vg), g_a):
        assert torch.equal(g.grad, a.to(torch.bfloat16))

    for fp8 in (False, True):
        q, kc, vc, lens, _ = _decode_case(hd, 8, 4, fp8, None)
        o_a = _decode_call(q, kc, vc, lens, scale, 0)
        o_b = _decode_call(q, kc, vc, lens, scale, 0, 0.0)
        o_f = F.attn_decode(q, kc, vc, lens, softcap=None)
        assert torch.equal(o_a, o_b) and torch.equal(o_a, o_f)


def test_attn_varlen_dispatch_softcap():
    """F.attn_varlen with a cap is the HIP autograd function, forward and
    MFMA backward, not the padded torch path."""
    hd, nq, nkv = 256, 4, 4
    q, k, v, dout, cu, refs = _bwd_case(hd, nq, nkv, None)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = F.attn_varlen(qg, kg, vg, cu, max(BWD_LENS), True, None, softcap=2.0)
    assert type(out.grad_fn).__name__.startswith("_AttnVarlenFn"), out.grad_fn
    out.backward(dout)
    for name, g, r in zip(("dq", "dk", "dv"), (qg, kg, vg), refs[2.0]):
        print("dispatch softcap", name, "max err", _maxerr(g.grad.float().cpu(), r))
        # bf16 gradients: test_attn_varlen_dispatch_hd256's bound
        torch.testing.assert_close(g.grad.float().cpu(), r, atol=8e-2, rtol=8e-2)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_attn_decode_dispatch_softcap(fp8, monkeypatch):
    q, kc, vc, lens, refs = _decode_case(256, 8, 1, fp8, None)

    def boom(*a, **kw):
        raise AssertionError("attn_decode_ref called with a softcap")

    monkeypatch.setattr(F, "attn_decode_ref", boom)
    out = F.attn_decode(q, kc, vc, lens, softcap=2.0)
    torch.testing.assert_close(out.float().cpu(), refs[2.0], **FWD_TOL)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
HD = 256


def _gemma2_cfg(attn_cap=2.0, final_cap=3.0):
    import realhf_amd.models.hf as hf_reg

    cfg = hf_reg.get_family("gemma2").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=1, head_dim=HD,
        vocab_size=256, intermediate_dim=512, sliding_window=8,
        attn_logit_softcap=attn_cap, final_logit_softcap=final_cap,
        query_pre_attn_scalar=144.0,
    )
    cfg.family = "gemma2"
    assert cfg.sliding_window_layers == [True, False]
    return cfg


def _gemma2_model(seed, **kw):
    from realhf_amd.models.real_model import ReaLModel

    cfg = _gemma2_cfg(**kw)
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init()
    with torch.no_grad():
        # the four norms of a block must differ for a swap to show
        for k, p in m._params.items():
            if k.endswith("ln.weight"):
                p.copy_(torch.randn_like(p) * 0.3)
    return cfg, m


def test_fused_decode_gemma2_matches_eager(monkeypatch):
    """A gemma2 layer keeps the fused decode block (no new blocker), and it
    agrees with the eager decode route: logits and appended K/V.  Contexts of
    20 and 12 are past the window of the sliding layer."""
    from realhf_amd.models import layers

    cfg, model = _gemma2_model(11)
    assert layers.fused_decode_blocker(cfg, torch.bfloat16, True, False) is None
    bs, maxlen = 3, 32
    torch.manual_seed(3)
    kv = [tuple((torch.randn(bs, maxlen, 1, HD, device="cuda") * 0.5)
                .to(torch.bfloat16) for _ in range(2))
          for _ in range(cfg.n_layers)]
    kv2 = [(k.clone(), v.clone()) for k, v in kv]
    tokens = torch.randint(0, 256, (bs,), device="cuda")
    cache_seqlens = torch.tensor([5, 20, 12], dtype=torch.int32, device="cuda")

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
    print("gemma2 fused vs eager max |diff|",
          _maxerr(out_fused.float(), out_eager.float()), "max |logit|",
          out_eager.float().abs().max().item())
    assert out_eager.float().abs().max() <= 3.0  # the final cap
    torch.testing.assert_close(out_fused.float(), out_eager.float(),
                               atol=3e-2, rtol=3e-2)
    for (k1, v1), (k2, v2) in zip(kv, kv2):
        torch.testing.assert_close(k1.float(), k2.float(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(v1.float(), v2.float(), atol=2e-2, rtol=2e-2)


def _prompts():
    toks = torch.randint(0, 256, (24,), device="cuda")
    cu = torch.tensor([0, 12, 24], dtype=torch.int32, device="cuda")
    return toks, cu


def test_generate_gemma2_captures_decode_graph(monkeypatch):
    """generate() captures the decode hipGraph for gemma2, and the graph's
    tokens equal those of eager decode (contexts 12 -> 20, window 8)."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models.generation import generate

    cfg, m = _gemma2_model(44)
    toks, cu = _prompts()
    g = GenerationHyperparameters(max_new_tokens=8, greedy=True,
                                  use_hip_graph=True)
    out_graph = generate(m, toks, cu, g)
    assert m._gen_session[1].decoder.graph is not None
    m._gen_session = None  # fresh session for the failing-capture run
    monkeypatch.setenv("REALHF_AMD_FORCE_GRAPH_FAIL", "1")
    out_eager = generate(m, toks, cu, g)
    assert m._gen_session[1].decoder.graph is None
    assert torch.equal(out_graph.gen_tokens, out_eager.gen_tokens)


def test_generate_gemma2_fp8_not_downgraded():
    """kv_quant and weight_quant stay on for gemma2: no blocker, no warning,
    FP8 caches and weights in the session, finite log-probs."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models import generation

    cfg, m = _gemma2_model(45)
    toks, cu = _prompts()
    g = GenerationHyperparameters(max_new_tokens=8, greedy=True,
                                  use_hip_graph=True, kv_quant="fp8_e4m3",
                                  weight_quant="fp8_e4m3")
    assert generation.effective_kv_quant(m, g) == "fp8_e4m3"
    assert generation.effective_weight_quant(m, g) == "fp8_e4m3"
    out = generation.generate(m, toks, cu, g)
    assert not getattr(m, "_kv_quant_warned", False)
    assert not getattr(m, "_weight_quant_warned", False)
    sess = m._gen_session[1]
    assert isinstance(sess.kv_caches[0][0], F.Fp8KVCache)
    assert sess.fp8 is not None and sess.fp8.nbytes() > 0
    assert sess.decoder.graph is not None
    assert torch.isfinite(out.gen_logprobs.float()).all()


def test_sft_step_gemma2():
    """One SFT train step (forward, capped MFMA backward, optimizer)."""
    import realhf_amd.interfaces  # noqa: F401
    from realhf_amd.api.config import Abstraction, ModelName
    from realhf_amd.api.data import SequenceSample
    from realhf_amd.api.model import (FinetuneSpec, Model, make_backend,
                                      make_interface)

    cfg, m = _gemma2_model(0)
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


# ---------------------------------------------------------------------------
# accuracy through a whole model
# ---------------------------------------------------------------------------
GRAD_KEYS = ("attn.ln.weight", "attn.post_ln.weight", "mlp.ln.weight",
             "mlp.post_ln.weight", "ln_f.weight", "attn.wq.weight",
             "attn.wk.weight", "attn.wv.weight", "attn.wo.weight",
             "mlp.gate.weight", "mlp.up.weight", "mlp.down.weight")


def _own_tensors(m):
    """Give every parameter its own leaf tensor (same values), so that each
    of q/k/v and gate/up gets its gradient (through the merged view of
    adjacent flat-buffer regions only the first of them does)."""
    for k in list(m._params):
        m._params[k] = m._params[k].detach().clone().requires_grad_(True)


def _logits_and_grads(m, toks, cu, max_seqlen):
    from realhf_amd.utils.functional import gather_packed_shifted_log_probs

    for p in m._params.values():
        p.grad = None
    logits = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=max_seqlen)
    gather_packed_shifted_log_probs(logits, cu, toks).mean().backward()
    out = {k: p.grad.float().cpu().clone() for k, p in m._params.items()
           if k.split(".", 1)[1] in GRAD_KEYS}
    out["logits"] = logits.detach().float().cpu()
    return out


def _errors_vs_fp32(attn_cap, final_cap):
    from realhf_amd.models.real_model import ReaLModel

    cfg, m = _gemma2_model(7, attn_cap=attn_cap, final_cap=final_cap)
    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
    _own_tensors(m)
    _own_tensors(m32)
    rng = np.random.RandomState(3)
    lens = [33, 64]
    toks = torch.from_numpy(rng.randint(0, cfg.vocab_size, size=sum(lens))).long()
    cu = torch.tensor([0, 33, 97], dtype=torch.int32)
    g32 = _logits_and_grads(m32, toks, cu, 64)
    g = _logits_and_grads(m, toks.cuda(), cu.cuda(), 64)
    assert len(g32) == 11 * cfg.n_layers + 2  # + ln_f and the logits
    errs = {}
    for k in g32:
        assert g32[k].norm() > 0 and torch.isfinite(g[k]).all(), k
        errs[k] = ((g[k] - g32[k]).norm() / g32[k].norm()).item()
    return errs


def test_gemma2_accuracy_no_worse_than_uncapped():
    """Prefill logits and per-tensor gradients of the mean next-token
    log-prob (packed 33 + 64) against an fp32 CPU copy, e = |g - g32| / |g32|.
    The same model with both caps off runs the kernels as they were; the caps
    add rounding of their own but should not make a tensor systematically
    worse: e_capped <= 2 * e_uncapped + 1e-3."""
    capped = _errors_vs_fp32(2.0, 3.0)
    plain = _errors_vs_fp32(None, None)
    bad = []
    for k in capped:
        print(f"error vs fp32  {k:24s} capped {capped[k]:.3e}  "
              f"uncapped {plain[k]:.3e}")
        if not capped[k] <= 2 * plain[k] + 1e-3:
            bad.append((k, capped[k], plain[k]))
    assert not bad, bad
