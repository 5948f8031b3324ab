"""Qwen3's per-head QK RMSNorm on the HIP path: the fused norm + RoPE kernel
(forward, backward), the decode epilogue with the norm inside
(rope_qkv_decode_norm / rope_qkv_decode_fp8_norm), and a tiny qwen3 model
against the REALHF_AMD_NO_QK_NORM_OPS kill switch and an fp32 CPU copy.

Kernel references are fp32 on the CPU from the same 16-bit inputs.
Tolerances are the project's for these ops: forward and decode atol = rtol =
3e-2 (rope in test_ops_gpu), dx atol = rtol = 1e-1 and dw atol 0.5, rtol 5e-2
(test_rmsnorm_fwd_bwd).  Weights are 1 + 0.5 N(0,1), different for q and k;
inputs are N(0,1) scaled per head row by factors from 0.1 to 10, so a missing
or head-crossing reduction is far outside the tolerance, and every kernel test
checks that the un-normed kernel on the same input is."""
import contextlib
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

EPS = 1e-6
KILL = "REALHF_AMD_NO_QK_NORM_OPS"
TOL = dict(atol=3e-2, rtol=3e-2)
HEADS = [(1, 1), (4, 2), (8, 1)]
TABLE_LEN = 512


def _tables(hd):
    cos, sin = F.rotary_cache.get(hd, TABLE_LEN, 10000.0, "cpu")
    return cos, sin, cos.cuda(), sin.cuda()


def _scaled_rows(g, rows, nh, hd):
    """N(0,1) [rows, nh, hd], head row r scaled by one of 7 factors 0.1..10."""
    x = torch.randn(rows, nh, hd, generator=g)
    fac = 10.0 ** torch.linspace(-1, 1, 7)
    return x * fac[(torch.arange(rows * nh) % 7).reshape(rows, nh, 1)]


def _weights(g, hd, dtype):
    q_w = (1 + 0.5 * torch.randn(hd, generator=g)).to(dtype)
    k_w = (1 + 0.5 * torch.randn(hd, generator=g)).to(dtype)
    assert not torch.equal(q_w, k_w)
    return q_w, k_w


_CASES = {}


def _case(total, nq, nkv, hd, dtype):
    """Inputs and the fp32 CPU reference (forward, rstd, gradients); computed
    once, shared by the tests and never modified."""
    key = (total, nq, nkv, hd, dtype)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(hash(key[:4]) % 2**31)
    nh = nq + 2 * nkv
    x = _scaled_rows(g, total, nh, hd)
    x[0, 0] = 0  # a q row of zeros
    merged = x.reshape(total, nh * hd).to(dtype)
    q_w, k_w = _weights(g, hd, dtype)
    a = (total + 1) // 2  # two packed sequences with their own positions
    pos = torch.cat([torch.arange(a), torch.arange(total - a)])
    gq = torch.randn(total, nq, hd, generator=g).to(dtype)
    gk = torch.randn(total, nkv, hd, generator=g).to(dtype)
    cos, sin, _, _ = _tables(hd)
    leaf = merged.float().requires_grad_(True)
    w32 = [q_w.float().requires_grad_(True), k_w.float().requires_grad_(True)]
    q, k, _ = leaf.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    q, k = q.reshape(total, nq, hd), k.reshape(total, nkv, hd)
    qo, ko = F.qk_norm_rope_ref(q, k, *w32, EPS, cos, sin, pos)
    torch.autograd.backward([qo, ko], [gq.float(), gk.float()])
    rstd = torch.rsqrt(torch.cat([q, k], 1).detach().pow(2).mean(-1) + EPS)
    out = dict(merged=merged, q_w=q_w, k_w=k_w, pos=pos, gq=gq, gk=gk,
               qo=qo.detach(), ko=ko.detach(), rstd=rstd, dx=leaf.grad,
               dqw=w32[0].grad, dkw=w32[1].grad)
    _CASES[key] = out
    return out


def _views(merged, nq, nkv, hd):
    total = merged.shape[0]
    q, k, _ = merged.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    return q.reshape(total, nq, hd), k.reshape(total, nkv, hd)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nkv", HEADS)
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_qk_norm_rope_fwd(hd, nq, nkv):
    _, _, cos, sin = _tables(hd)
    for dtype in (torch.bfloat16, torch.float16):
        for total in (1, 17, 330):
            c = _case(total, nq, nkv, hd, dtype)
            what = f"fwd hd{hd} {nq}/{nkv} total{total} {dtype}"
            merged = c["merged"].cuda()
            q, k = _views(merged, nq, nkv, hd)
            assert total == 1 or not q.is_contiguous()
            q_w, k_w, pos = c["q_w"].cuda(), c["k_w"].cuda(), c["pos"].cuda()
            qo, ko, rstd = C.qk_norm_rope_fwd(q, k, q_w, k_w, EPS, cos, sin,
                                              pos, True)
            assert qo.is_contiguous() and ko.is_contiguous()
            assert rstd.shape == (total, nq + nkv) and rstd.dtype == torch.float32
            # contiguous inputs (as LoRA produces): the same bits
            qo2, ko2, rstd2 = C.qk_norm_rope_fwd(
                q.contiguous(), k.contiguous(), q_w, k_w, EPS, cos, sin, pos,
                True)
            assert torch.equal(qo, qo2) and torch.equal(ko, ko2), what
            assert torch.equal(rstd, rstd2), what
            for name, got, want in (("q", qo, c["qo"]), ("k", ko, c["ko"])):
                err = (got.float().cpu() - want).abs().max().item()
                print(what, name, "max err", err, "max |ref|",
                      want.abs().max().item())
                torch.testing.assert_close(got.float().cpu(), want, **TOL,
                                           msg=lambda m: f"{what} {name}: {m}")
            rel = ((rstd.cpu() - c["rstd"]).abs() / c["rstd"]).max().item()
            print(what, "rstd max rel err", rel)
            assert rel <= 1e-5, what
            # the row of zeros: zeros out, finite rstd
            assert torch.isfinite(rstd).all()
            assert int((qo[0, 0] != 0).sum()) == 0, what
            # the un-normed kernel on the same input is outside the tolerance
            # (k: at total 1 with one q head the only q row is the zero row)
            for x, want in ((q, c["qo"]), (k, c["ko"])):
                if int((x != 0).sum()) == 0:
                    continue
                plain = C.rope_fwd(x.contiguous(), cos, sin, pos, False, False)
                assert not torch.allclose(plain.float().cpu(), want, **TOL), what
            # the public op takes the same route
            with torch.no_grad():
                qo3, ko3 = F.qk_norm_rope(q, k, q_w, k_w, EPS, cos, sin, pos)
            assert torch.equal(qo3, qo) and torch.equal(ko3, ko), what


def test_qk_norm_rope_no_rotation_and_fallbacks(monkeypatch):
    """cos = None skips the rotation inside the kernel; interleaved rotary,
    another head dim and the kill switch take the torch reference."""
    nq, nkv, hd, total = 4, 2, 128, 17
    c = _case(total, nq, nkv, hd, torch.bfloat16)
    _, _, cos, sin = _tables(hd)
    q, k = _views(c["merged"].cuda(), nq, nkv, hd)
    q_w, k_w, pos = c["q_w"].cuda(), c["k_w"].cuda(), c["pos"].cuda()
    seen = []
    real = C.qk_norm_rope_fwd
    monkeypatch.setattr(C, "qk_norm_rope_fwd",
                        lambda *a: seen.append(1) or real(*a))
    with torch.no_grad():
        qo, ko = F.qk_norm_rope(q, k, q_w, k_w, EPS, None, None, None)
        assert len(seen) == 1
        qr, kr = F.qk_norm_rope_ref(q.float().cpu(), k.float().cpu(),
                                    q_w.float().cpu(), k_w.float().cpu(), EPS,
                                    None, None, None)
        torch.testing.assert_close(qo.float().cpu(), qr, **TOL)
        torch.testing.assert_close(ko.float().cpu(), kr, **TOL)
        F.qk_norm_rope(q, k, q_w, k_w, EPS, cos, sin, pos, interleaved=True)
        F.qk_norm_rope(q[..., :96], k[..., :96], q_w[:96], k_w[:96], EPS,
                       None, None, None)
        monkeypatch.setenv(KILL, "1")
        qk, kk = F.qk_norm_rope(q, k, q_w, k_w, EPS, cos, sin, pos)
        assert len(seen) == 1
        monkeypatch.delenv(KILL)
        qh, kh = F.qk_norm_rope(q, k, q_w, k_w, EPS, cos, sin, pos)
        assert len(seen) == 2
        torch.testing.assert_close(qh.float(), qk.float(), **TOL)
        torch.testing.assert_close(kh.float(), kk.float(), **TOL)


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nkv", HEADS)
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_qk_norm_rope_bwd(hd, nq, nkv):
    _, _, cos, sin = _tables(hd)
    for dtype in (torch.bfloat16, torch.float16):
        for total in (1, 17, 330):
            c = _case(total, nq, nkv, hd, dtype)
            what = f"bwd hd{hd} {nq}/{nkv} total{total} {dtype}"
            pos = c["pos"].cuda()
            gq, gk = c["gq"].cuda(), c["gk"].cuda()
            runs = []
            for _ in range(2):
                leaf = c["merged"].cuda().requires_grad_(True)
                q_w = c["q_w"].cuda().requires_grad_(True)
                k_w = c["k_w"].cuda().requires_grad_(True)
                q, k = _views(leaf, nq, nkv, hd)
                qo, ko = F.qk_norm_rope(q, k, q_w, k_w, EPS, cos, sin, pos)
                torch.autograd.backward([qo, ko], [gq, gk])
                runs.append((leaf.grad, q_w.grad, k_w.grad))
            (dx, dqw, dkw), (dx2, dqw2, dkw2) = runs
            # no atomics: the same bits twice
            assert torch.equal(dqw, dqw2) and torch.equal(dkw, dkw2), what
            assert torch.equal(dx, dx2), what
            nqk = (nq + nkv) * hd
            assert int((dx[:, nqk:] != 0).sum()) == 0, what  # v gets nothing
            for name, got, want, tol in (
                    ("dq/dk", dx[:, :nqk], c["dx"][:, :nqk],
                     dict(atol=1e-1, rtol=1e-1)),
                    ("dw_q", dqw, c["dqw"], dict(atol=0.5, rtol=5e-2)),
                    ("dw_k", dkw, c["dkw"], dict(atol=0.5, rtol=5e-2))):
                err = (got.float().cpu() - want).abs().max().item()
                print(what, name, "max err", err, "max |ref|",
                      want.abs().max().item())
                torch.testing.assert_close(got.float().cpu(), want, **tol,
                                           msg=lambda m: f"{what} {name}: {m}")
            # the un-normed backward (the conjugate rotation alone) is
            # outside the tolerance
            plain = C.rope_fwd(gk, cos, sin, pos, False, True)
            assert not torch.allclose(
                plain.float().cpu().reshape(total, -1),
                c["dx"][:, nq * hd:nqk], atol=1e-1, rtol=1e-1), what


def test_bwd_uses_more_than_one_workgroup():
    """total 330 at the smallest geometry is already several 256-thread
    workgroups, so the dw partial rows of more than one are summed."""
    assert 330 * (1 + 1) * (64 // 8) > 2 * 256


# ---------------------------------------------------------------------------
# decode epilogue
# ---------------------------------------------------------------------------
MAXLEN = 20
SENTINEL = 7.0


def _decode_ref(x32, q_w, k_w, lens, cos, sin, nq, nkv, norm=True):
    """x32 [bs, nh, hd] fp32 (bias added) -> q [bs, nq, hd], k, v rows."""
    qk = x32[:, :nq + nkv]
    if norm:
        w = torch.cat([q_w.float().expand(nq, -1), k_w.float().expand(nkv, -1)])
        qk = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + EPS) * w
    qk = F.apply_rotary_ref(qk, cos, sin, torch.tensor(lens) - 1)
    return qk[:, :nq], qk[:, nq:], x32[:, nq + nkv:]


def _filled_fp8(bs, nkv, hd):
    c = F.Fp8KVCache.zeros(bs, MAXLEN, nkv, hd, "cuda")
    c.codes.view(torch.uint8).fill_(0x55)
    c.scale.fill_(-1.0)
    return c


def _check_fp8(cache, dense_rows, seq, pos, what):
    """cache at (seq, pos) == quantize_rows_e4m3_ref(dense_rows), codes and
    scale bits; every other position still holds the fill."""
    n, nkv, hd = dense_rows.shape
    q, s = F.quantize_rows_e4m3_ref(dense_rows.cpu().reshape(-1, hd))
    q = q.view(torch.uint8).reshape(n, nkv, hd)
    s = s.reshape(n, nkv)
    codes, scale = cache.codes.view(torch.uint8).cpu(), cache.scale.cpu()
    assert torch.equal(codes[seq, pos], q), what
    assert torch.equal(scale[seq, :, pos].view(torch.int32),
                       s.view(torch.int32)), what
    touched = torch.zeros(codes.shape[:2], dtype=torch.bool)
    touched[seq, pos] = True
    assert int((codes[~touched] != 0x55).sum()) == 0, what
    assert int((scale.transpose(1, 2)[~touched] != -1.0).sum()) == 0, what


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_rope_qkv_decode_norm(hd):
    nq, nkv = 4, 2
    nh = nq + 2 * nkv
    qkvd = nh * hd
    cos, sin, cosg, sing = _tables(hd)
    g = torch.Generator().manual_seed(hd)
    q_w, k_w = _weights(g, hd, torch.bfloat16)
    qwg, kwg = q_w.cuda(), k_w.cuda()
    bias_all = (0.5 * torch.randn(qkvd, generator=g)).to(torch.bfloat16)
    for bs in (1, 3, 16):
        lens = list(range(1, bs + 1))  # all different, including 1
        cs = torch.tensor(lens, dtype=torch.int32, device="cuda")
        seq, pos = torch.arange(bs), torch.tensor(lens) - 1
        written = torch.zeros(bs, MAXLEN, dtype=torch.bool)
        written[seq, pos] = True
        base = _scaled_rows(g, bs, nh, hd).reshape(bs, qkvd)
        for nks in (0, 1, 3, 8):  # 0: the bf16 input
            if nks == 0:
                qkv = base.to(torch.bfloat16).cuda()
                summed = qkv.float().cpu()
            else:
                parts = torch.randn(nks, bs, qkvd, generator=g)
                parts[0] += base - parts.sum(0)
                qkv = parts.cuda().contiguous()
                acc = qkv[0].clone()
                for s in range(1, nks):  # the kernel's order: slab 0, +1, ...
                    acc = acc + qkv[s]
                summed = acc.cpu()
            for bias in (None, bias_all):
                what = f"decode hd{hd} bs{bs} nks{nks} bias={bias is not None}"
                bg = None if bias is None else bias.cuda()
                x32 = summed if bias is None else summed + bias.float()
                q_ref, k_ref, v_ref = _decode_ref(
                    x32.reshape(bs, nh, hd), q_w, k_w, lens, cos, sin, nq, nkv)
                kc = torch.full((bs, MAXLEN, nkv, hd), SENTINEL,
                                dtype=torch.bfloat16, device="cuda")
                vc = kc.clone()
                q = C.rope_qkv_decode_norm(qkv, bg, kc, vc, cs, cosg, sing, nq,
                                           True, qwg, kwg, EPS)
                kcc, vcc = kc.cpu(), vc.cpu()
                for name, got, want in (("q", q.cpu(), q_ref),
                                        ("k", kcc[seq, pos], k_ref),
                                        ("v", vcc[seq, pos], v_ref)):
                    err = (got.float() - want).abs().max().item()
                    print(what, name, "max err", err)
                    torch.testing.assert_close(
                        got.float(), want, **TOL,
                        msg=lambda m: f"{what} {name}: {m}")
                # every other cache row keeps the sentinel
                for cache in (kcc, vcc):
                    assert int((cache[~written] != SENTINEL).sum()) == 0, what
                # the un-normed kernel is outside the tolerance
                kc0, vc0 = torch.zeros_like(kc), torch.zeros_like(vc)
                q0 = C.rope_qkv_decode(qkv, bg, kc0, vc0, cs, cosg, sing, nq,
                                       True)
                assert not torch.allclose(q0.float().cpu(), q_ref, **TOL), what
                assert not torch.allclose(kc0.cpu()[seq, pos].float(), k_ref,
                                          **TOL), what
                assert torch.equal(vc0.cpu()[seq, pos], vcc[seq, pos]), what
                if nks > 1:
                    # slabs == one fp32 slab holding their sequential sum,
                    # bit for bit (test_decode_chains_gpu's criterion)
                    kc1, vc1 = (torch.zeros_like(kc) for _ in range(2))
                    kc2, vc2 = (torch.zeros_like(kc) for _ in range(2))
                    q1 = C.rope_qkv_decode_norm(
                        summed.cuda()[None].contiguous(), bg, kc1, vc1, cs,
                        cosg, sing, nq, True, qwg, kwg, EPS)
                    q2 = C.rope_qkv_decode_norm(qkv, bg, kc2, vc2, cs, cosg,
                                                sing, nq, True, qwg, kwg, EPS)
                    assert torch.equal(q1, q2) and torch.equal(kc1, kc2), what
                    assert torch.equal(vc1, vc2), what
                # FP8 cache form: bit for bit the reference quantization of
                # the rows the bf16-cache form wrote from the same input
                k8, v8 = _filled_fp8(bs, nkv, hd), _filled_fp8(bs, nkv, hd)
                q8 = C.rope_qkv_decode_fp8_norm(
                    qkv, bg, k8.codes, k8.scale, v8.codes, v8.scale, cs, cosg,
                    sing, nq, True, qwg, kwg, EPS)
                assert torch.equal(q8, q), what
                _check_fp8(k8, kcc[seq, pos], seq, pos, what + " K")
                _check_fp8(v8, vcc[seq, pos], seq, pos, what + " V")


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _qwen3(seed, device="cuda", dtype=torch.bfloat16):
    """2 layers, hidden 256, 4 heads on 2 kv heads, hd 128; q/k norm weights
    1 + 0.5 N(0,1), different from each other."""
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("qwen3").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=4, n_kv_heads=2, head_dim=128,
        vocab_size=256, intermediate_dim=512)
    cfg.family = "qwen3"
    assert cfg.qk_rmsnorm
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device=device, dtype=dtype)
    m.random_init(std=0.05)
    with torch.no_grad():
        for k, t in m._params.items():
            if "q_ln" in k or "k_ln" in k:
                t.copy_(1 + 0.5 * torch.randn_like(t))
    return cfg, m


def _fp32_copy(cfg, m):
    from realhf_amd.models.real_model import ReaLModel

    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
    return m32


def _packed(lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(0, 256, (sum(lens),), generator=g)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    return toks.cuda(), cu.cuda()


def _own_tensors(m):
    """Every parameter its own leaf (same values), so that each gets its
    gradient: q/k/v and gate/up then run as separate GEMMs joined by cat."""
    for k in list(m._params):
        m._params[k] = m._params[k].detach().clone().requires_grad_(True)


def _loss_grads(m, toks, cu, max_seqlen):
    from realhf_amd.utils.functional import gather_packed_shifted_log_probs

    for p in m._params.values():
        p.grad = None
    logits = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=max_seqlen)
    gather_packed_shifted_log_probs(logits, cu, toks).mean().backward()
    return logits.detach().float().cpu(), {
        k: p.grad.float().cpu().clone() for k, p in m._params.items()
        if p.grad is not None}


def test_qwen3_training_no_worse_than_torch_path(monkeypatch):
    """Packed 33 + 64 tokens: prefill logits of the HIP path against the kill
    switch, and the gradients of the mean next-token log-prob against an fp32
    CPU copy, per tensor: e_hip <= 2 * e_torch + 1e-3, e = |g - g32| / |g32|
    (test_gemma_gradients_no_worse_than_torch_path's criterion)."""
    monkeypatch.delenv(KILL, raising=False)
    cfg, m = _qwen3(seed=7)
    m32 = _fp32_copy(cfg, m)
    _own_tensors(m)
    _own_tensors(m32)
    toks, cu = _packed([33, 64])
    lg32, g32 = _loss_grads(m32, toks.cpu(), cu.cpu(), 64)
    seen = []
    real = C.qk_norm_rope_bwd
    monkeypatch.setattr(C, "qk_norm_rope_bwd",
                        lambda *a: seen.append(1) or real(*a))
    lg_hip, g_hip = _loss_grads(m, toks, cu, 64)
    assert len(seen) == cfg.n_layers
    monkeypatch.setenv(KILL, "1")
    lg_torch, g_torch = _loss_grads(m, toks, cu, 64)
    assert len(seen) == cfg.n_layers
    print("qwen3 prefill logits hip vs kill switch max |diff|",
          (lg_hip - lg_torch).abs().max().item(), "max |logit|",
          lg_torch.abs().max().item())
    assert lg_torch.abs().max() > 0.1
    torch.testing.assert_close(lg_hip, lg_torch, **TOL)
    assert set(g_hip) == set(g_torch) == set(g32)
    assert sum("q_ln" in k or "k_ln" in k for k in g32) == 2 * cfg.n_layers
    assert len(g32) >= 11 * cfg.n_layers + 2

    def rel(g, k):
        return ((g[k] - g32[k]).norm() / g32[k].norm()).item()

    bad = []
    for k in g32:
        e_hip, e_torch = rel(g_hip, k), rel(g_torch, k)
        print(f"grad error vs fp32  {k:22s} hip {e_hip:.3e}  torch {e_torch:.3e}")
        assert g32[k].norm() > 0 and np.isfinite(e_hip)
        if not e_hip <= 2 * e_torch + 1e-3:
            bad.append((k, e_hip, e_torch))
    assert not bad, bad


LENS = [12, 9, 5]
STEPS = 8  # decode steps after the prefill


def _prompts(device="cuda"):
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 256, (sum(LENS),), generator=g)
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    return toks.to(device), cu.to(device)


def _gconfig(graph, kv=None, weight=None):
    from realhf_amd.api.model import GenerationHyperparameters

    return GenerationHyperparameters(max_new_tokens=STEPS + 1, greedy=True,
                                     use_hip_graph=graph, kv_quant=kv,
                                     weight_quant=weight)


def _generate_logged(monkeypatch, m, gconfig, forced=None):
    """generate(), returning (output, [STEPS + 1, bs, V] logits the sampler
    saw).  forced [bs, STEPS + 1]: sample these tokens instead (teacher
    forcing, so two runs stay on one token path)."""
    from realhf_amd.models import generation as genmod

    seen = []
    real = genmod._sample_from_logits

    def spy(logits, *a, **kw):
        tokens, logp, mask = real(logits, *a, **kw)
        if forced is not None:
            tokens = forced[:, len(seen)]
            logp = torch.log_softmax(logits, -1).gather(
                -1, tokens.unsqueeze(-1)).squeeze(-1)
        seen.append(logits.clone())
        return tokens, logp, mask

    with monkeypatch.context() as mp:
        mp.setattr(genmod, "_sample_from_logits", spy)
        out = genmod.generate(m, *_prompts(), gconfig)
    return out, torch.stack(seen)


APPENDS = ("rope_qkv_decode", "rope_qkv_decode_fp8", "rope_qkv_decode_norm",
           "rope_qkv_decode_fp8_norm")


def _spy_appends(monkeypatch):
    seen = {n: 0 for n in APPENDS}

    def spy(name):
        real = getattr(C, name)

        def f(*a):
            seen[name] += 1
            return real(*a)

        monkeypatch.setattr(C, name, f)

    for n in APPENDS:
        spy(n)
    return seen


def test_qwen3_decode_matches_kill_switch(monkeypatch):
    """Prefill + 8 greedy steps: the fused route with the norm inside the
    append kernel (one rope_qkv_decode_norm per layer and step, none of the
    un-normed one), the same tokens with and without the captured graph, and
    step logits within 3e-2 + 3e-2 |ref| of the kill switch on those tokens."""
    monkeypatch.delenv(KILL, raising=False)
    cfg, m = _qwen3(seed=44)
    L = cfg.n_layers
    seen = _spy_appends(monkeypatch)
    out_eager, lg_hip = _generate_logged(monkeypatch, m, _gconfig(False))
    assert m._gen_session[1].decoder.graph is None
    assert seen == {"rope_qkv_decode": 0, "rope_qkv_decode_fp8": 0,
                    "rope_qkv_decode_norm": STEPS * L,
                    "rope_qkv_decode_fp8_norm": 0}
    assert out_eager.gen_tokens.shape == (3, STEPS + 1)

    m._gen_session = None
    out_graph, _ = _generate_logged(monkeypatch, m, _gconfig(True))
    assert m._gen_session[1].decoder.graph is not None
    assert torch.equal(out_graph.gen_tokens, out_eager.gen_tokens)
    assert seen["rope_qkv_decode"] == 0

    for v in APPENDS:
        seen[v] = 0
    monkeypatch.setenv(KILL, "1")
    out_ref, lg_ref = _generate_logged(monkeypatch, m, _gconfig(False),
                                       forced=out_eager.gen_tokens)
    monkeypatch.delenv(KILL)
    # the kill switch: torch norm in front of the un-normed kernel
    assert seen["rope_qkv_decode"] == STEPS * L
    assert seen["rope_qkv_decode_norm"] == 0
    assert torch.equal(out_ref.gen_tokens, out_eager.gen_tokens)
    print("qwen3 decode kernels vs kill switch: max |diff|",
          (lg_hip - lg_ref).abs().max().item(), "max |logit|",
          lg_ref.abs().max().item())
    assert lg_ref.abs().max() > 0.1
    torch.testing.assert_close(lg_hip, lg_ref, **TOL)
    # the norm matters to this model: without it the logits move
    for k, t in m._params.items():
        if "q_ln" in k or "k_ln" in k:
            assert (t.float() - 1).abs().max() > 0.3


def _teacher_forced(m, forced, fp8_kv=False, fp8_w=None):
    """Prefill, then STEPS decode steps on forced[:, :STEPS]; returns the
    log-prob of forced[:, 1:] under each decode step's logits [bs, STEPS]."""
    dev = m.flat_param.device
    cfg = m.config
    toks, cu = _prompts(dev)
    bs = len(LENS)
    if fp8_kv:
        kv = [tuple(F.Fp8KVCache.zeros(bs, 128, cfg.n_kv_heads, cfg.head_dim,
                                       dev) for _ in range(2))
              for _ in range(cfg.n_layers)]
    else:
        kv = [tuple(torch.zeros(bs, 128, cfg.n_kv_heads, cfg.head_dim,
                                dtype=m.dtype, device=dev) for _ in range(2))
              for _ in range(cfg.n_layers)]
    m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=max(LENS), kv_caches=kv)
    seqlens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    forced = forced.to(dev)
    logps = []
    for t in range(STEPS):
        seqlens = seqlens + 1
        with (fp8_w.installed() if fp8_w is not None
              else contextlib.nullcontext()):
            lg = m(packed_input_ids=forced[:, t], kv_caches=kv,
                   cache_seqlens=seqlens, decode=True)
        lp = torch.log_softmax(lg.float(), -1)
        logps.append(lp.gather(-1, forced[:, t + 1].unsqueeze(-1)).squeeze(-1))
    return torch.stack(logps, 1).cpu()


@pytest.mark.parametrize("mode", ["kv", "weight"])
def test_qwen3_fp8_generation(monkeypatch, mode):
    """kv_quant / weight_quant = fp8_e4m3 generate on the fused route with
    the norm inside the append kernel, and the mean |d log-prob| of 8
    teacher-forced tokens against the unquantised run is no worse than the
    fp32 CPU model with the reference quantisers gives: e_kernel <=
    2 * e_ref + 1e-3 (test_fp8_kv_gpu / test_fp8_decode_gpu)."""
    from realhf_amd.models.generation import Fp8DecodeWeights

    for v in (KILL, "REALHF_AMD_GEN_KV_QUANT", "REALHF_AMD_GEN_WEIGHT_QUANT",
              "REALHF_AMD_NO_FP8_KV", "REALHF_AMD_NO_FP8_SKINNY"):
        monkeypatch.delenv(v, raising=False)
    cfg, m = _qwen3(seed=47)
    L = cfg.n_layers
    out, _ = _generate_logged(monkeypatch, m, _gconfig(False))
    forced = out.gen_tokens  # sampled by the unquantised bf16 model
    seen = _spy_appends(monkeypatch)
    m._gen_session = None
    kw = dict(kv="fp8_e4m3") if mode == "kv" else dict(weight="fp8_e4m3")
    outq, _ = _generate_logged(monkeypatch, m, _gconfig(True, **kw))
    assert m._gen_session[1].decoder.graph is not None
    assert outq.gen_tokens.shape == (3, STEPS + 1)
    normed = "rope_qkv_decode_fp8_norm" if mode == "kv" else "rope_qkv_decode_norm"
    assert seen[normed] > 0  # captured once, replayed after
    assert sum(seen.values()) == seen[normed]
    m._gen_session = None
    outq_eager, _ = _generate_logged(monkeypatch, m, _gconfig(False, **kw))
    assert seen[normed] > STEPS * L and sum(seen.values()) == seen[normed]
    assert torch.equal(outq_eager.gen_tokens, outq.gen_tokens)

    m32 = _fp32_copy(cfg, m)
    with torch.no_grad():
        if mode == "kv":
            args, args32 = dict(fp8_kv=True), dict(fp8_kv=True)
        else:
            fp8, fp8_32 = Fp8DecodeWeights(m), Fp8DecodeWeights(m32)
            fp8.refresh()
            fp8_32.refresh()
            args, args32 = dict(fp8_w=fp8), dict(fp8_w=fp8_32)
        lp_bf16 = _teacher_forced(m, forced)
        lp_q = _teacher_forced(m, forced, **args)
        lp_32 = _teacher_forced(m32, forced)
        lp_32_q = _teacher_forced(m32, forced, **args32)
    e_kernel = (lp_q - lp_bf16).abs().mean().item()
    e_ref = (lp_32_q - lp_32).abs().mean().item()
    print(f"qwen3 mean |dlogp| fp8 {mode} vs unquantised: kernel path "
          f"{e_kernel:.4e}, fp32 CPU reference {e_ref:.4e}")
    assert e_ref > 0 and e_kernel > 0
    assert e_kernel <= 2 * e_ref + 1e-3
