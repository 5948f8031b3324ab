"""FP8 weight-only decode on the GPU: the e4m3 row quantizer against its
CPU definition (bitwise), the fp8-weight skinny GEMM (exact decode of every
code, fp32 reference, slab consumers), and a tiny llama through generate():
kernel path against the REALHF_AMD_NO_FP8_SKINNY reference, captured graph
against eager, refresh under a captured graph, dispatch, and the
quantization error a user sees against the same error of the fp32 CPU
reference."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

KILL = "REALHF_AMD_NO_FP8_SKINNY"
ENV = "REALHF_AMD_GEN_WEIGHT_QUANT"


def _u8(t):
    return t.view(torch.uint8).cpu()


# ---------------------------------------------------------------------------
# quantizer: bitwise against the CPU reference
# ---------------------------------------------------------------------------
def _quant_case(name):
    torch.manual_seed(31)
    if name == "one_row":
        return (0.02 * torch.randn(1, 64)).to(torch.bfloat16)
    if name == "one_vector":  # K = 8: one active lane per row
        return torch.randn(3, 8).to(torch.bfloat16)
    if name == "strided_rows":  # stride(0) > K, as a view into flat_param is
        buf = (0.02 * torch.randn(64, 4096 + 64)).to(torch.bfloat16)
        buf[7] = 0  # an all-zero row
        return buf[:, :4096]
    if name == "ragged_outlier":  # 5.4 trips of the column loop
        w = (0.02 * torch.randn(5, 11008)).to(torch.bfloat16)
        w[2, 4097] = 20.0  # 1000x outlier: the rest scale to ~0.45 |z|
        w[4, 5] = 640.0  # 2^15 x: most of the rest land in e4m3 subnormals
        return w
    if name == "unaligned":  # rows off the 16-byte grid: the scalar kernel
        buf = torch.randn(3, 66).to(torch.bfloat16)
        return buf[:, 1:65]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_row", "one_vector", "strided_rows",
                                  "ragged_outlier", "unaligned"])
def test_quantizer_bitwise(name):
    w = _quant_case(name)
    q_ref, s_ref = F.quantize_rows_e4m3_ref(w)
    wg_buf = w._base.cuda() if w._base is not None else w.cuda()
    wg = wg_buf.as_strided(w.shape, w.stride(), w.storage_offset())
    assert wg.stride() == w.stride() and torch.equal(wg.cpu(), w)
    q, s = C.quantize_rows_e4m3(wg)
    assert q.dtype == torch.float8_e4m3fn and q.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (w.shape[0],)
    bad_s = (s.cpu().view(torch.int32) != s_ref.view(torch.int32)).sum().item()
    bad_q = (_u8(q) != q_ref.view(torch.uint8)).sum().item()
    print("quantizer", name, tuple(w.shape), "scale mismatches", bad_s,
          "code mismatches", bad_q)
    assert bad_s == 0 and bad_q == 0
    assert int(((_u8(q) & 0x7F) == 0x7F).sum()) == 0  # no NaN codes
    if name == "strided_rows":
        assert s[7] == 1.0 and int(_u8(q)[7].sum()) == 0
    if name == "ragged_outlier":
        sub = (_u8(q) & 0x78) == 0  # exponent field 0: subnormal or zero
        nz = (_u8(q) & 0x7F) != 0
        print("subnormal codes per row", (sub & nz).sum(1).tolist())
        assert (sub & nz)[2].sum() > 50 and (sub & nz)[4].sum() > 11008 // 4
        for r in (2, 4):  # the outliers themselves: 448
            assert (_u8(q)[r] & 0x7F).max() == 0x7E

    # in-place form: same bits into caller-owned buffers, addresses kept
    q2 = torch.full(w.shape, 0x55, dtype=torch.uint8, device="cuda").view(
        torch.float8_e4m3fn)
    s2 = torch.full((w.shape[0],), -1.0, device="cuda")
    pq, ps = q2.data_ptr(), s2.data_ptr()
    out = F.quantize_rows_e4m3(wg, out=(q2, s2))
    assert out[0] is q2 and out[1] is s2
    assert (q2.data_ptr(), s2.data_ptr()) == (pq, ps)
    assert torch.equal(_u8(q2), _u8(q)) and torch.equal(s2, s)


# ---------------------------------------------------------------------------
# GEMM: every finite code decodes exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2], ids=["body", "remainder"])
def test_every_code_decodes_exactly(splitk):
    """q cycles through the 254 finite e4m3 codes (subnormals included),
    scale = 1, x rows are one-hot, so each output is one weight, exactly.
    K = 256 in one slice runs the 4-load body once; in two slices only the
    64-deep remainder loop.  Row m of call c is hot at k = 16 m + (c + m) %
    16: every call touches every 64-block and every g (the lane owning
    k-range [16 g, 16 g + 16) of a block is m % 4) and both halves of the
    16-byte load; the 16 calls together read all of q."""
    N, K, M = 64, 256, 16
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    assert codes.numel() == 254
    q8 = codes[torch.arange(N * K) % 254].view(N, K)
    q = q8.cuda().view(torch.float8_e4m3fn)
    want = q8.view(torch.float8_e4m3fn).float()  # [N, K], CPU decode
    assert torch.isfinite(want).all() and want.abs().max() == 448.0
    scale = torch.ones(N, device="cuda")
    ws = torch.empty(4 * M * N, dtype=torch.float32, device="cuda")
    got = torch.full((N, K), float("nan"))
    for c in range(16):
        hot = torch.tensor([16 * m + (c + m) % 16 for m in range(M)])
        x = torch.zeros(M, K)
        x[torch.arange(M), hot] = 1.0
        parts = C.skinny_gemm_fp8_nc(x.to(torch.bfloat16).cuda(), q, scale, ws,
                                     splitk)
        assert parts.shape == (splitk, M, N) and parts.dtype == torch.float32
        got[:, hot] = parts.sum(0).cpu().t()
    bad = got != want
    print("exact decode, splitk", splitk, "mismatches", int(bad.sum()))
    assert int(bad.sum()) == 0
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# GEMM against fp8_linear_ref in fp32
# ---------------------------------------------------------------------------
def _gemm_case(M, K, N, seed=15):
    torch.manual_seed(seed)
    x = (torch.randn(M, K) * 0.3).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.3).to(torch.bfloat16)
    res = (torch.randn(M, N) * 0.3).to(torch.bfloat16)
    q, _ = F.quantize_rows_e4m3_ref(w)
    # 2^-8 .. 2^7 by row index: a mis-indexed scale cannot hide
    scale = torch.pow(2.0, (torch.arange(N) % 16 - 8).float())
    ref = F.fp8_linear_ref(x.float(), q, scale)  # fp32, CPU
    return x, q, scale, res, ref


@pytest.mark.parametrize("M,K,N,splitk", [
    (16, 64, 64, 8),  # one k-step, nks = 1
    (5, 192, 128, 2),  # uneven slices (128 + 64), M tail
    (1, 4096, 4096, 8),  # two trips of the body per slice
    (16, 11008, 4096, 16),  # 704-deep slices: body twice, remainder 3x
])
def test_fp8_gemm_matches_ref(M, K, N, splitk):
    """Tolerance of test_skinny_gemm_with_residual at its 0.3-scaled
    inputs; both sides see the same q, so no quantization error is in it."""
    x, q, scale, res, ref = _gemm_case(M, K, N)
    xg, qg, sg, rg = x.cuda(), q.cuda(), scale.cuda(), res.cuda()
    ws = torch.empty(32 * 16 * N, dtype=torch.float32, device="cuda")
    parts = C.skinny_gemm_fp8_nc(xg, qg, sg, ws, splitk)
    kslice = (K // splitk + 63) // 64 * 64
    assert parts.shape == ((K + kslice - 1) // kslice, M, N)
    got_nc = parts.sum(0).cpu()
    out = C.skinny_gemm_fp8(xg, qg, sg, ws, splitk, None)
    out_r = C.skinny_gemm_fp8(xg, qg, sg, ws, splitk, rg)
    assert out.dtype == out_r.dtype == torch.bfloat16 and out.shape == (M, N)
    out, out_r = out.float().cpu(), out_r.float().cpu()
    for name, got, want in (("nc", got_nc, ref), ("combined", out, ref),
                            ("residual", out_r, ref + res.float())):
        print("fp8 gemm", (M, K, N, splitk), name, "max |err|",
              (got - want).abs().max().item(), "max |ref|",
              want.abs().max().item())
    assert ref.abs().max() > 1
    torch.testing.assert_close(got_nc, ref, atol=0.3, rtol=3e-2)
    torch.testing.assert_close(out, ref, atol=0.3, rtol=3e-2)
    torch.testing.assert_close(out_r, ref + res.float(), atol=0.3, rtol=3e-2)


def test_fp8_dispatch_and_kill_switch(monkeypatch):
    """maybe_skinny_linear / skinny_linear_nc with a pair reach the fp8
    entry points; the kill switch sends the same pair to fp8_linear_ref."""
    x, q, scale, res, ref = _gemm_case(16, 256, 128)
    xg, pair, rg = x.cuda(), (q.cuda(), scale.cuda()), res.cuda()
    w = torch.empty(128, 256, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        parts = F.skinny_linear_nc(xg, w, fp8=pair)
        assert parts.dim() == 3 and parts.dtype == torch.float32
        torch.testing.assert_close(parts.sum(0).cpu(), ref, atol=0.3, rtol=3e-2)
        out = F.maybe_skinny_linear(xg, w, residual=rg, fp8=pair)
        monkeypatch.setenv(KILL, "1")
        assert F.skinny_linear_nc(xg, w, fp8=pair) is None
        out_ref = F.maybe_skinny_linear(xg, w, residual=rg, fp8=pair)
        # K = 96 is not a multiple of 64: no fp8 kernel, the reference runs
        monkeypatch.delenv(KILL)
        pair96 = (pair[0][:, :96].contiguous(), pair[1])
        assert F.skinny_linear_nc(xg[:, :96].contiguous(), w, fp8=pair96) is None
    assert out.dtype == out_ref.dtype == torch.bfloat16
    torch.testing.assert_close(out.float(), out_ref.float(), atol=0.3, rtol=3e-2)
    with pytest.raises(RuntimeError, match="K % 64"):
        C.skinny_gemm_fp8_nc(xg[:, :96].contiguous(), pair96[0], pair96[1],
                             torch.empty(1 << 16, device="cuda"), 2)


def test_fp8_slab_consumers_match_combined():
    """fp8 slabs consumed in the add_rmsnorm / swiglu / rope prologues match
    combine-then-consume, at test_slab_consumers_match_combined's
    tolerances: the row scale is already in the slabs."""
    torch.manual_seed(17)
    M, H, I = 16, 1024, 1408
    ws = torch.empty(32 * 16 * 2 * I, dtype=torch.float32, device="cuda")

    def pair(n, k):
        w = (torch.randn(n, k, device="cuda") * 0.05).to(torch.bfloat16)
        return C.quantize_rows_e4m3(w)

    qo, so = pair(H, H)
    attn = (torch.randn(M, H, device="cuda") * 0.3).to(torch.bfloat16)
    x = (torch.randn(M, H, device="cuda") * 0.3).to(torch.bfloat16)
    g = torch.randn(H, device="cuda").to(torch.bfloat16)
    o_bf = C.skinny_gemm_fp8(attn, qo, so, ws, 8, None)
    ref_h2, ref_x2 = C.add_rmsnorm_fwd(o_bf, x, g, 1e-5)
    parts = C.skinny_gemm_fp8_nc(attn, qo, so, ws, 8)
    assert parts.shape == (8, M, H)
    h2, x2 = C.add_rmsnorm_fwd(parts, x, g, 1e-5)
    torch.testing.assert_close(x2.float(), ref_x2.float(), atol=0.1, rtol=5e-2)
    torch.testing.assert_close(h2.float(), ref_h2.float(), atol=0.1, rtol=5e-2)
    assert ref_h2.float().abs().max() > 0.5

    qgu, sgu = pair(2 * I, H)
    gu_bf = C.skinny_gemm_fp8(h2, qgu, sgu, ws, 8, None)
    ref_act = C.swiglu_fwd(gu_bf)
    act = C.swiglu_fwd(C.skinny_gemm_fp8_nc(h2, qgu, sgu, ws, 8))
    torch.testing.assert_close(act.float(), ref_act.float(), atol=0.1, rtol=5e-2)
    assert ref_act.float().abs().max() > 0.1

    nq = nkv = 4
    hd = 128
    qq, sq = pair((nq + 2 * nkv) * hd, H)
    hin = (torch.randn(M, H, device="cuda") * 0.3).to(torch.bfloat16)
    maxlen = 64
    kc1 = torch.zeros(M, maxlen, nkv, hd, dtype=torch.bfloat16, device="cuda")
    vc1, kc2, vc2 = (torch.zeros_like(kc1) for _ in range(3))
    lens = torch.randint(1, maxlen, (M,), dtype=torch.int32, device="cuda")
    pos = torch.arange(maxlen, device="cuda", dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device="cuda").float() / hd))
    ang = pos[:, None] * inv[None, :]
    cosb, sinb = ang.cos().contiguous(), ang.sin().contiguous()
    qkv_bf = C.skinny_gemm_fp8(hin, qq, sq, ws, 8, None)
    q_ref = C.rope_qkv_decode(qkv_bf, None, kc1, vc1, lens, cosb, sinb, nq, True)
    qkv_parts = C.skinny_gemm_fp8_nc(hin, qq, sq, ws, 8)
    q = C.rope_qkv_decode(qkv_parts, None, kc2, vc2, lens, cosb, sinb, nq, True)
    torch.testing.assert_close(q.float(), q_ref.float(), atol=0.1, rtol=5e-2)
    torch.testing.assert_close(kc2.float(), kc1.float(), atol=0.1, rtol=5e-2)
    torch.testing.assert_close(vc2.float(), vc1.float(), atol=0.1, rtol=5e-2)
    assert q_ref.float().abs().max() > 0.5


# ---------------------------------------------------------------------------
# model level: tiny llama, 2 layers, hidden 256, intermediate 512, hd 128
# ---------------------------------------------------------------------------
LENS = [12, 9, 5]
STEPS = 8  # decode steps after the prefill


def _llama(seed=44, device="cuda", dtype=torch.bfloat16):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=2, head_dim=128,
        vocab_size=256, intermediate_dim=512,
    )
    cfg.family = "llama"
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device=device, dtype=dtype)
    m.random_init(std=0.05)
    return cfg, m


def _prompts(device="cuda"):
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 256, (sum(LENS),), generator=g)
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    return toks.to(device), cu.to(device)


def _gconfig(quant, graph):
    from realhf_amd.api.model import GenerationHyperparameters

    return GenerationHyperparameters(max_new_tokens=STEPS + 1, greedy=True,
                                     use_hip_graph=graph, weight_quant=quant)


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


def test_model_fp8_kernel_matches_kill_switch(monkeypatch):
    """Prefill + 8 greedy decode steps: skinny_gemm_fp8 against
    fp8_linear_ref on the same (q, scale), at the bound
    test_gemma_model_matches_torch_path uses for two bf16 orderings of the
    same math; a captured graph samples what eager decode samples."""
    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _llama()
    out_hip, lg_hip = _generate_logged(monkeypatch, m, _gconfig("fp8_e4m3", True))
    sess = m._gen_session[1]
    assert sess.decoder.graph is not None and sess.fp8 is not None
    assert out_hip.gen_tokens.shape == (3, STEPS + 1)

    m._gen_session = None  # fresh session for the failing-capture run
    monkeypatch.setenv("REALHF_AMD_FORCE_GRAPH_FAIL", "1")
    out_eager, lg_eager = _generate_logged(monkeypatch, m,
                                           _gconfig("fp8_e4m3", True))
    assert m._gen_session[1].decoder.graph is None
    assert torch.equal(out_hip.gen_tokens, out_eager.gen_tokens)
    monkeypatch.delenv("REALHF_AMD_FORCE_GRAPH_FAIL")

    monkeypatch.setenv(KILL, "1")
    out_ref, lg_ref = _generate_logged(monkeypatch, m, _gconfig("fp8_e4m3", False),
                                       forced=out_hip.gen_tokens)
    monkeypatch.delenv(KILL)
    assert torch.equal(out_ref.gen_tokens, out_hip.gen_tokens)
    print("fp8 kernel vs fp8_linear_ref: max |diff|",
          (lg_hip - lg_ref).abs().max().item(), "max |logit|",
          lg_ref.abs().max().item())
    assert lg_ref.abs().max() > 0.1
    torch.testing.assert_close(lg_hip, lg_ref, atol=3e-2, rtol=3e-2)


def test_model_refresh_under_captured_graph(monkeypatch):
    """A second generate() after an in-place change of flat_param replays
    the SAME captured graph and sees the new weights, because the session
    re-quantizes into the buffers the graph reads."""
    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _llama(seed=45)
    g = _gconfig("fp8_e4m3", True)
    _, lg0 = _generate_logged(monkeypatch, m, g)
    sess = m._gen_session[1]
    graph = sess.decoder.graph
    assert graph is not None
    addrs = [q.data_ptr() for d in sess.fp8.pairs for q, _ in d.values()]
    with torch.no_grad():
        torch.manual_seed(3)
        for k, t in m._params.items():
            if t.ndim == 2 and (".attn." in k or ".mlp." in k):
                t.add_(0.03 * torch.randn_like(t))
    out1, lg1 = _generate_logged(monkeypatch, m, g)
    assert m._gen_session[1] is sess and sess.decoder.graph is graph
    assert addrs == [q.data_ptr() for d in sess.fp8.pairs for q, _ in d.values()]
    # what a fresh eager session computes from the new weights
    m._gen_session = None
    _, lg_fresh = _generate_logged(monkeypatch, m, _gconfig("fp8_e4m3", False),
                                   forced=out1.gen_tokens)
    change = (lg1[1:] - lg0[1:]).abs().max().item()
    print("decode logits: change after the weight update", change,
          "graph replay vs fresh eager session",
          (lg1 - lg_fresh).abs().max().item())
    assert change > 0.1
    torch.testing.assert_close(lg1, lg_fresh, atol=3e-2, rtol=3e-2)


def test_model_dispatch(monkeypatch):
    """weight_quant="none" (and the unset default) calls exactly the bf16
    entry points the parent commit called and nothing of the fp8 path;
    "fp8_e4m3" moves the four block projections, and only those, to the fp8
    entry points."""
    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _llama(seed=46)
    names = ("skinny_gemm", "skinny_gemm_nc", "skinny_gemm_fp8",
             "skinny_gemm_fp8_nc", "quantize_rows_e4m3_", "quantize_rows_e4m3")
    seen = {n: [] for n in names}

    def spy(name):
        real = getattr(C, name)

        def f(*a):
            seen[name].append(a)
            return real(*a)

        monkeypatch.setattr(C, name, f)

    for n in names:
        spy(n)
    L = cfg.n_layers
    outs = {}
    for quant in (None, "none"):
        for v in seen.values():
            v.clear()
        m._gen_session = None
        outs[quant], _ = _generate_logged(monkeypatch, m, _gconfig(quant, False))
        # per decode step: qkv, wo, gate/up slabs per layer; down (residual
        # folded) per layer and the output head through the combine
        assert len(seen["skinny_gemm_nc"]) == STEPS * 3 * L
        assert len(seen["skinny_gemm"]) == STEPS * (L + 1)
        for n in names[2:]:
            assert not seen[n], n
        assert m._gen_session[1].fp8 is None
    assert torch.equal(outs[None].gen_logprobs, outs["none"].gen_logprobs)

    for v in seen.values():
        v.clear()
    _generate_logged(monkeypatch, m, _gconfig("fp8_e4m3", False))
    assert len(seen["skinny_gemm_fp8_nc"]) == STEPS * 3 * L
    assert len(seen["skinny_gemm_fp8"]) == STEPS * L
    assert all(a[5] is not None for a in seen["skinny_gemm_fp8"])  # the fold
    assert len(seen["quantize_rows_e4m3_"]) == 4 * L  # one refresh
    assert not seen["skinny_gemm_nc"]
    assert len(seen["skinny_gemm"]) == STEPS  # the output head stays bf16
    # the environment variable alone selects it, too
    for v in seen.values():
        v.clear()
    monkeypatch.setenv(ENV, "fp8_e4m3")
    _generate_logged(monkeypatch, m, _gconfig(None, False))
    assert len(seen["skinny_gemm_fp8_nc"]) == STEPS * 3 * L
    assert len(seen["quantize_rows_e4m3_"]) == 4 * L  # refreshed again


def _teacher_forced(m, forced, fp8=None):
    """Prefill, then STEPS decode steps on forced[:, :STEPS]; returns the
    log-prob of forced[:, 1:] under each decode step's logits [bs, STEPS].
    fp8: an Fp8DecodeWeights to install for the decode steps."""
    dev = m.flat_param.device
    cfg = m.config
    toks, cu = _prompts(dev)
    bs = len(LENS)
    kv = [tuple(torch.zeros(bs, 128, cfg.n_kv_heads, cfg.head_dim,
                            dtype=m.dtype, device=dev) for _ in range(2))
          for _ in range(cfg.n_layers)]
    m(packed_input_ids=toks, cu_seqlens=cu, max_seqlen=max(LENS), kv_caches=kv)
    seqlens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    forced = forced.to(dev)
    logps = []
    for t in range(STEPS):
        seqlens = seqlens + 1
        with (fp8.installed() if fp8 is not None else contextlib.nullcontext()):
            lg = m(packed_input_ids=forced[:, t], kv_caches=kv,
                   cache_seqlens=seqlens, decode=True)
        lp = torch.log_softmax(lg.float(), -1)
        logps.append(lp.gather(-1, forced[:, t + 1].unsqueeze(-1)).squeeze(-1))
    return torch.stack(logps, 1).cpu()


def test_quantization_error_no_worse_than_fp32_reference(monkeypatch):
    """Mean |log-prob difference| of the sampled tokens between fp8 and bf16
    decode, against the same quantity for fp8_linear_ref in fp32 on the CPU
    (an fp32 copy of the model, with and without the quantized weights).
    Both see the same quantization; the kernel path adds only bf16 rounding
    in a different order, so e_kernel <= 2 * e_ref + 1e-3, the rule of
    test_gemma_gradients_no_worse_than_torch_path."""
    from realhf_amd.models.generation import Fp8DecodeWeights
    from realhf_amd.models.real_model import ReaLModel

    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _llama(seed=47)
    out, _ = _generate_logged(monkeypatch, m, _gconfig("none", False))
    forced = out.gen_tokens  # [bs, STEPS + 1], sampled by the bf16 model
    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
        fp8 = Fp8DecodeWeights(m)
        fp8.refresh()
        fp8_32 = Fp8DecodeWeights(m32)
        fp8_32.refresh()
        for d, d32 in zip(fp8.pairs, fp8_32.pairs):  # the same quantization
            assert set(d) == set(d32) == {"qkv", "wo", "gu", "down"}
            for k in d:
                assert torch.equal(_u8(d[k][0]), _u8(d32[k][0]))
        lp_bf16 = _teacher_forced(m, forced)
        lp_fp8 = _teacher_forced(m, forced, fp8)
        lp_32 = _teacher_forced(m32, forced)
        lp_32_fp8 = _teacher_forced(m32, forced, fp8_32)
    e_kernel = (lp_fp8 - lp_bf16).abs().mean().item()
    e_ref = (lp_32_fp8 - lp_32).abs().mean().item()
    print(f"mean |dlogp| fp8 vs unquantized: kernel path {e_kernel:.4e}, "
          f"fp32 CPU reference {e_ref:.4e}")
    assert e_ref > 0 and e_kernel > 0
    assert e_kernel <= 2 * e_ref + 1e-3
