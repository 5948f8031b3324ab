"""Gemma's norm and GeGLU on the HIP path: the 1 + w weight mode of the
RMSNorm kernels, the GeGLU kernels (forward, backward, split-K slab
consumer), the Python dispatch with its REALHF_AMD_NO_GEMMA_OPS kill switch,
and a gemma model against the torch path and an fp32 CPU copy.  Kernel
references are fp32 on the CPU from the same bf16 inputs."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

HD = 256
EPS = 1e-6
KILL = "REALHF_AMD_NO_GEMMA_OPS"


# ---------------------------------------------------------------------------
# RMSNorm, 1 + w weight mode
# ---------------------------------------------------------------------------
def _norm_case(rows, H, dtype, seed=1):
    torch.manual_seed(seed)
    x = torch.randn(rows, H).to(dtype)
    w = (0.1 * torch.randn(H)).to(dtype)
    g = torch.randn(rows, H).to(dtype)
    x_ref = x.float().clone().requires_grad_(True)
    w_ref = w.float().clone().requires_grad_(True)
    ref = F.gemma_rms_norm_ref(x_ref, w_ref, EPS)
    ref.backward(g.float())
    return x, w, g, ref.detach(), x_ref.grad, w_ref.grad


@pytest.mark.parametrize("rows,H,dtype", [
    (1, 8, torch.bfloat16),  # one vector, one active lane
    (7, 128, torch.bfloat16),  # fewer columns than threads
    (300, 2048, torch.bfloat16),  # a full trip of the column loop
    (33, 3072, torch.bfloat16),  # 1.5 trips: ragged last trip
    (600, 128, torch.bfloat16),  # > 512 rows: grid-stride rows, dw partials
    (33, 3072, torch.float32),  # 4 elements per lane, 3 trips
], ids=lambda v: str(v).replace("torch.", ""))
def test_gemma_rmsnorm_fwd_bwd(rows, H, dtype):
    """Tolerances of test_rmsnorm_fwd_bwd: the same math with a shifted
    weight."""
    x, w, g, ref, dx_ref, dw_ref = _norm_case(rows, H, dtype)
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    out = F._RMSNormFn.apply(xg, wg, EPS, True)
    out.backward(g.cuda())
    for name, got, want in (("out", out, ref), ("dx", xg.grad, dx_ref),
                            ("dw", wg.grad, dw_ref)):
        err = (got.detach().float().cpu() - want).abs().max().item()
        print("gemma rmsnorm", (rows, H), dtype, name, "max err", err)
    torch.testing.assert_close(out.float().cpu(), ref, atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(xg.grad.float().cpu(), dx_ref, atol=1e-1, rtol=1e-1)
    torch.testing.assert_close(wg.grad.float().cpu(), dw_ref, atol=0.5, rtol=5e-2)


def _gain_error(out, ref):
    keep = ref.abs() > 1e-3
    return (out.float().cpu()[keep] / ref[keep] - 1).mean().item()


def test_gemma_weight_sum_is_fp32():
    """Every w = bf16(0.01).  1 + w rounded to bf16 is 1.0078125, a gain
    error of -2.2e-3; the fp32 sum leaves only the output rounding, whose
    mean is +7e-5 on these inputs.  Bound: 5e-4."""
    torch.manual_seed(5)
    rows, H = 64, 2048
    x = torch.randn(rows, H).to(torch.bfloat16)
    w = torch.full((H,), 0.01).to(torch.bfloat16)
    ref = F.gemma_rms_norm_ref(x.float(), w.float(), EPS)
    out, _ = C.gemma_rmsnorm_fwd(x.cuda(), w.cuda(), EPS)
    e = _gain_error(out, ref)
    print("gemma_rmsnorm_fwd mean(out/ref - 1)", e)
    assert abs(e) <= 5e-4, e

    r = torch.randn(rows, H).to(torch.bfloat16)
    out2, s2 = C.gemma_add_rmsnorm_fwd(x.cuda(), r.cuda(), w.cuda(), EPS)
    assert torch.equal(s2.cpu(), (x.float() + r.float()).to(torch.bfloat16))
    ref2 = F.gemma_rms_norm_ref(s2.float().cpu(), w.float(), EPS)
    e2 = _gain_error(out2, ref2)
    print("gemma_add_rmsnorm_fwd mean(out/ref - 1)", e2)
    assert abs(e2) <= 5e-4, e2


def test_plain_weight_mode_untouched():
    """The old call forms still mean plain RMSNorm: with w = 0 they return
    zeros, and the gemma entry points return the normalised input."""
    torch.manual_seed(6)
    x = torch.randn(9, 256).to(torch.bfloat16)
    r = torch.randn(9, 256).to(torch.bfloat16)
    w = torch.zeros(256, dtype=torch.bfloat16)
    xc, rc, wc = x.cuda(), r.cuda(), w.cuda()
    one = torch.ones(256)

    out, rstd = C.rmsnorm_fwd(xc, wc, EPS)
    assert torch.count_nonzero(out) == 0
    gout, grstd = C.gemma_rmsnorm_fwd(xc, wc, EPS)
    assert torch.equal(rstd, grstd)
    torch.testing.assert_close(gout.float().cpu(),
                               F.rms_norm_ref(x.float(), one, EPS),
                               atol=5e-2, rtol=5e-2)

    out, s = C.add_rmsnorm_fwd(xc, rc, wc, EPS)
    assert torch.count_nonzero(out) == 0
    gout, gs = C.gemma_add_rmsnorm_fwd(xc, rc, wc, EPS)
    assert torch.equal(s, gs)
    torch.testing.assert_close(gout.float().cpu(),
                               F.rms_norm_ref(gs.float().cpu(), one, EPS),
                               atol=5e-2, rtol=5e-2)

    # backward: dx through w = 0 is zero in plain mode only
    g = torch.randn(9, 256).to(torch.bfloat16).cuda()
    dx, _ = C.rmsnorm_bwd(g, xc, wc, rstd)
    assert torch.count_nonzero(dx) == 0
    gdx, _ = C.gemma_rmsnorm_bwd(g, xc, wc, rstd)
    assert torch.count_nonzero(gdx) > 0


# ---------------------------------------------------------------------------
# GeGLU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,I", [(1, 8), (257, 1024), (5, 24576)])
def test_geglu_fwd_bwd(tokens, I):
    """Gate 3 * randn reaches both tails of the GELU.  Tolerances of
    test_swiglu_fwd_bwd."""
    torch.manual_seed(3)
    gu = torch.randn(tokens, 2 * I)
    gu[:, :I] *= 3
    gu = gu.to(torch.bfloat16)
    g = torch.randn(tokens, I).to(torch.bfloat16)
    ref_in = gu.float().clone().requires_grad_(True)
    ref = F.geglu_ref(ref_in)
    ref.backward(g.float())
    out = C.geglu_fwd(gu.cuda())
    dgu = C.geglu_bwd(g.cuda(), gu.cuda())
    print("geglu", (tokens, I), "fwd max err",
          (out.float().cpu() - ref).abs().max().item(), "bwd max err",
          (dgu.float().cpu() - ref_in.grad).abs().max().item())
    torch.testing.assert_close(out.float().cpu(), ref.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(dgu.float().cpu(), ref_in.grad, atol=5e-2, rtol=5e-2)
    # the autograd function saves gate_up and gives the same two results
    gug = gu.cuda().requires_grad_(True)
    out2 = F.geglu(gug)
    assert type(out2.grad_fn).__name__.startswith("_GeGLUFn"), out2.grad_fn
    out2.backward(g.cuda())
    assert torch.equal(out2, out) and torch.equal(gug.grad, dgu)


def test_geglu_saturated_tails():
    """__expf overflows to +inf for large negative gates: the forward is
    -0/0 there and the gate itself for large positive ones, and the backward
    forms no inf * 0."""
    gates = [-30, -12, -6, -0.0, 0, 6, 12, 30]
    gu = torch.tensor([gates + [1.0] * 8], dtype=torch.bfloat16).cuda()
    dy = torch.ones(1, 8, dtype=torch.bfloat16).cuda()
    out = C.geglu_fwd(gu).float().cpu()[0]
    dgu = C.geglu_bwd(dy, gu).float().cpu()[0]
    d_gate, d_up = dgu[:8], dgu[8:]
    print("geglu tails fwd", out.tolist())
    print("geglu tails d_gate", d_gate.tolist(), "d_up", d_up.tolist())
    assert torch.isfinite(out).all() and torch.isfinite(dgu).all()
    assert (out[:3].abs() <= 1e-6).all(), out
    assert torch.equal(out[3:], torch.tensor([0.0, 0, 6, 12, 30])), out
    assert abs(d_gate[0].item()) <= 1e-3 and abs(d_gate[7].item() - 1) <= 1e-3
    assert abs(d_gate[3].item() - 0.5) <= 1e-3 and abs(d_gate[4].item() - 0.5) <= 1e-3
    torch.testing.assert_close(d_up, out, atol=1e-6, rtol=0)  # up = dy = 1


# ---------------------------------------------------------------------------
# split-K slab consumers
# ---------------------------------------------------------------------------
def test_gemma_slab_consumers_match_combined():
    """As test_slab_consumers_match_combined, at the smallest shapes
    skinny_gemm_nc accepts."""
    torch.manual_seed(17)
    M, H, I = 5, 256, 512
    ws = torch.empty(2 * 8 * 16 * 2 * I, dtype=torch.float32, device="cuda")
    wo = (torch.randn(H, H, device="cuda") * 0.05).to(torch.bfloat16)
    attn = (torch.randn(M, H, device="cuda") * 0.3).to(torch.bfloat16)
    x = (torch.randn(M, H, device="cuda") * 0.3).to(torch.bfloat16)
    g = (0.1 * torch.randn(H, device="cuda")).to(torch.bfloat16)
    o_bf = C.skinny_gemm(attn, wo, ws, 8, None)
    ref_h2, ref_x2 = C.gemma_add_rmsnorm_fwd(o_bf, x, g, EPS)
    parts = C.skinny_gemm_nc(attn, wo, ws, 8)
    assert parts.dim() == 3 and parts.shape[1:] == (M, H) and parts.shape[0] > 1
    h2, x2 = C.gemma_add_rmsnorm_fwd(parts, x, g, EPS)
    torch.testing.assert_close(x2.float(), ref_x2.float(), atol=0.1, rtol=5e-2)
    torch.testing.assert_close(h2.float(), ref_h2.float(), atol=0.1, rtol=5e-2)
    # and it is the 1 + w mode: the plain slab form scales by w ~ 0.1
    p_h2, _ = C.add_rmsnorm_fwd(C.skinny_gemm_nc(attn, wo, ws, 8), x, g, EPS)
    assert not torch.allclose(p_h2.float(), h2.float(), atol=0.1, rtol=5e-2)

    wgu = (torch.randn(2 * I, H, device="cuda") * 0.05).to(torch.bfloat16)
    gu_bf = C.skinny_gemm(h2, wgu, ws, 8, None)
    ref_act = C.geglu_fwd(gu_bf)
    gu_parts = C.skinny_gemm_nc(h2, wgu, ws, 8)
    assert gu_parts.dim() == 3 and gu_parts.dtype == torch.float32
    act = C.geglu_fwd(gu_parts)
    assert act.shape == (M, I) and act.dtype == torch.bfloat16
    torch.testing.assert_close(act.float(), ref_act.float(), atol=0.1, rtol=5e-2)
    ref = F.geglu_ref(gu_parts.sum(0))
    torch.testing.assert_close(act.float(), ref, atol=3e-2, rtol=3e-2)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _gemma_cfg(n_layers):
    import realhf_amd.models.hf as hf_reg

    cfg = hf_reg.get_family("gemma").make_test_config(
        n_layers=n_layers, hidden_dim=256, n_heads=2, n_kv_heads=1,
        head_dim=HD, vocab_size=256, intermediate_dim=512,
    )
    cfg.family = "gemma"
    return cfg


def _gemma_model(n_layers, seed):
    from realhf_amd.models.real_model import ReaLModel

    cfg = _gemma_cfg(n_layers)
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init()
    with torch.no_grad():  # norm weights: 0.1 * randn, as in the kernel tests
        for t in m._params.values():
            if t.ndim == 1:
                t.copy_(0.1 * torch.randn_like(t))
    return cfg, m


def _packed(lens, seed=0):
    rng = np.random.RandomState(seed)
    toks = torch.from_numpy(rng.randint(0, 256, size=sum(lens))).long().cuda()
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32,
                      device="cuda")
    return toks, cu


def _decode_inputs(cfg, seed=9):
    torch.manual_seed(seed)
    bs, maxlen = 3, 32
    kv = [tuple(0.3 * torch.randn(bs, maxlen, 1, HD, device="cuda").to(torch.bfloat16)
                for _ in range(2)) for _ in range(cfg.n_layers)]
    tokens = torch.randint(0, 256, (bs,), device="cuda")
    cache_seqlens = torch.tensor([5, 9, 2], dtype=torch.int32, device="cuda")
    return tokens, kv, cache_seqlens


def _decode(m, tokens, kv, cache_seqlens):
    kv = [(k.clone(), v.clone()) for k, v in kv]
    return m(packed_input_ids=tokens, kv_caches=kv,
             cache_seqlens=cache_seqlens, decode=True)


def test_gemma_dispatch_and_kill_switch(monkeypatch):
    """A gemma layer never reaches the torch norm or GeGLU, and its decode
    step is the three fused launches of a llama layer: add+norm on the
    o-projection's slabs, the activation on the gate/up slabs, the residual
    folded into the down projection.  The kill switch undoes all of it."""
    cfg, m = _gemma_model(1, seed=12)
    toks, cu = _packed([33, 20])
    dec = _decode_inputs(cfg)
    seen = {}

    def spy(mod, name):
        real = getattr(mod, name)
        seen[name] = []

        def f(*a, **kw):
            seen[name].append(a)
            return real(*a, **kw)

        monkeypatch.setattr(mod, name, f)

    for name in ("gemma_rmsnorm_fwd", "gemma_add_rmsnorm_fwd", "geglu_fwd",
                 "skinny_gemm"):
        spy(C, name)

    def slab_calls(name):
        return [a for a in seen[name]
                if a[0].dim() == 3 and a[0].dtype == torch.float32]

    def folds():
        return [a for a in seen["skinny_gemm"] if a[4] is not None]

    with monkeypatch.context() as mp, torch.no_grad():
        def boom(*a, **kw):
            raise AssertionError("torch gemma reference reached on the GPU")

        mp.setattr(F, "gemma_rms_norm_ref", boom)
        mp.setattr(F, "geglu_ref", boom)
        m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=33)
        # attn.ln and mlp.ln per layer, and ln_f
        assert len(seen["gemma_rmsnorm_fwd"]) == 2 * cfg.n_layers + 1
        assert len(seen["geglu_fwd"]) == cfg.n_layers
        for v in seen.values():
            v.clear()
        _decode(m, *dec)
        assert len(slab_calls("gemma_add_rmsnorm_fwd")) == cfg.n_layers
        assert len(seen["gemma_add_rmsnorm_fwd"]) == cfg.n_layers
        assert len(slab_calls("geglu_fwd")) == cfg.n_layers
        assert len(seen["geglu_fwd"]) == cfg.n_layers
        assert len(folds()) == cfg.n_layers
        # what is left for the stand-alone norm: attn.ln per layer, ln_f
        assert len(seen["gemma_rmsnorm_fwd"]) == cfg.n_layers + 1

    for v in seen.values():
        v.clear()
    spy(F, "gemma_rms_norm_ref")
    spy(F, "geglu_ref")
    monkeypatch.setenv(KILL, "1")
    with torch.no_grad():
        m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=33)
        _decode(m, *dec)
    for name in ("gemma_rmsnorm_fwd", "gemma_add_rmsnorm_fwd", "geglu_fwd"):
        assert not seen[name], name
    assert not folds()
    assert len(seen["gemma_rms_norm_ref"]) == 2 * (2 * cfg.n_layers + 1)
    assert len(seen["geglu_ref"]) == 2 * cfg.n_layers


def test_gemma_model_matches_torch_path(monkeypatch):
    """HIP norm/GeGLU against the kill switch on the same weights: packed
    forward and a decode step at the bound the fused-versus-eager gemma test
    uses for two bf16 orderings of the same math; greedy generation under a
    captured graph equals generation with the capture forced to fail."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models.generation import generate

    cfg, m = _gemma_model(2, seed=44)
    toks, cu = _packed([33, 64, 47])
    dec = _decode_inputs(cfg)
    with torch.no_grad():
        fwd_hip = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=64)
        dec_hip = _decode(m, *dec)
        monkeypatch.setenv(KILL, "1")
        fwd_torch = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=64)
        dec_torch = _decode(m, *dec)
        monkeypatch.delenv(KILL)
    for name, a, b in (("packed", fwd_hip, fwd_torch), ("decode", dec_hip, dec_torch)):
        print("gemma hip vs torch", name, "max |diff|",
              (a.float() - b.float()).abs().max().item(),
              "max |logit|", b.float().abs().max().item())
        assert b.float().abs().max() > 0.1
        torch.testing.assert_close(a.float(), b.float(), atol=3e-2, rtol=3e-2)

    ptoks, pcu = _packed([12, 12], seed=1)
    g = GenerationHyperparameters(max_new_tokens=8, greedy=True,
                                  use_hip_graph=True)
    out_graph = generate(m, ptoks, pcu, g)
    assert m._gen_session[1].decoder.graph is not None
    m._gen_session = None  # fresh session for the failing-capture run
    monkeypatch.setenv("REALHF_AMD_FORCE_GRAPH_FAIL", "1")
    out_eager = generate(m, ptoks, pcu, g)
    assert m._gen_session[1].decoder.graph is None
    assert torch.equal(out_graph.gen_tokens, out_eager.gen_tokens)


GRAD_KEYS = ("attn.ln.weight", "mlp.ln.weight", "ln_f.weight",
             "mlp.gate.weight", "mlp.up.weight")


def _own_tensors(m):
    """Give every parameter its own leaf tensor (same values).  The blocks
    then run gate/up and q/k/v as separate GEMMs joined by torch.cat, and
    every one of them gets its gradient: through the merged view of adjacent
    flat-buffer regions only the first of the merged parameters does."""
    for k in list(m._params):
        m._params[k] = m._params[k].detach().clone().requires_grad_(True)


def _loss_grads(m, toks, cu, max_seqlen):
    from realhf_amd.utils.functional import gather_packed_shifted_log_probs

    for p in m._params.values():
        p.grad = None
    logits = m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=max_seqlen)
    gather_packed_shifted_log_probs(logits, cu, toks).mean().backward()
    return {k: p.grad.float().cpu().clone() for k, p in m._params.items()
            if k.split(".", 1)[1] in GRAD_KEYS}


def test_gemma_gradients_no_worse_than_torch_path(monkeypatch):
    """Gradients of the mean next-token log-prob against an fp32 CPU copy of
    the model.  The HIP path and the torch bf16 path round the same fp32
    math in a different order, so neither should be systematically worse:
    e_hip <= 2 * e_torch + 1e-3 per tensor, e = |g - g32| / |g32|."""
    from realhf_amd.models.real_model import ReaLModel

    cfg, m = _gemma_model(2, seed=7)
    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
    _own_tensors(m)
    _own_tensors(m32)
    toks, cu = _packed([33, 64], seed=3)
    g32 = _loss_grads(m32, toks.cpu(), cu.cpu(), 64)
    g_hip = _loss_grads(m, toks, cu, 64)
    monkeypatch.setenv(KILL, "1")
    g_torch = _loss_grads(m, toks, cu, 64)
    assert len(g32) == 4 * cfg.n_layers + 1

    def rel(g, k):
        return ((g[k] - g32[k]).norm() / g32[k].norm()).item()

    bad = []
    for k in g32:
        e_hip, e_torch = rel(g_hip, k), rel(g_torch, k)
        print(f"grad error vs fp32  {k:20s} hip {e_hip:.3e}  torch {e_torch:.3e}")
        assert g32[k].norm() > 0 and np.isfinite(e_hip)
        if not e_hip <= 2 * e_torch + 1e-3:
            bad.append((k, e_hip, e_torch))
    assert not bad, bad
