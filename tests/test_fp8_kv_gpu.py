"""FP8 (e4m3) KV cache on the GPU: the quantizing decode append and prefill
store against the CPU quantizer (bitwise), decode attention over the codes
(exact decode of every V code, the fp32 CPU reference, poisoned positions
outside the attended range), and tiny models through generate(): dispatch,
kernels against the REALHF_AMD_NO_FP8_KV references, captured graph against
eager, and the quantization error a user sees against the same error of the
fp32 CPU reference."""
import copy
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box

KILL = "REALHF_AMD_NO_FP8_KV"
ENV = "REALHF_AMD_GEN_KV_QUANT"
WENV = "REALHF_AMD_GEN_WEIGHT_QUANT"


def _u8(t):
    return t.view(torch.uint8).cpu()


def _bits(t):
    return t.cpu().view(torch.int32)


def _rope_tables(maxlen, hd):
    pos = torch.arange(maxlen, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    ang = pos[:, None] * inv[None, :]
    return ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda()


def _filled(bs, maxlen, nkv, hd):
    """An fp8 cache whose every byte is 0x55 and every scale -1: what the
    kernels must leave alone."""
    c = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cuda")
    c.codes.view(torch.uint8).fill_(0x55)
    c.scale.fill_(-1.0)
    return c


def _check_cache(cache, dense_rows, seq, pos, what):
    """cache at (seq[i], pos[i]) == quantize_rows_e4m3_ref(dense_rows[i]),
    codes and scale bits; every other position still holds the fill."""
    n, nkv, hd = dense_rows.shape
    q, s = F.quantize_rows_e4m3_ref(dense_rows.cpu().reshape(-1, hd))
    q = q.view(torch.uint8).reshape(n, nkv, hd)
    s = s.reshape(n, nkv)
    codes, scale = _u8(cache.codes), cache.scale.cpu()
    got_q = codes[seq, pos]
    got_s = scale[seq, :, pos]
    bad_q = int((got_q != q).sum())
    bad_s = int((got_s.view(torch.int32) != s.view(torch.int32)).sum())
    touched = torch.zeros(codes.shape[:2], dtype=torch.bool)
    touched[seq, pos] = True
    stray_q = int((codes[~touched] != 0x55).sum())
    stray_s = int((scale.transpose(1, 2)[~touched] != -1.0).sum())
    print(what, "code mismatches", bad_q, "scale mismatches", bad_s,
          "touched elsewhere", stray_q, stray_s)
    assert bad_q == 0 and bad_s == 0 and stray_q == 0 and stray_s == 0
    assert int(((got_q & 0x7F) == 0x7F).sum()) == 0  # no NaN codes
    return got_q, got_s


# ---------------------------------------------------------------------------
# quantizing decode append: bitwise against the bf16 append + CPU quantizer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 5, 16])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_append_bitwise(hd, nq, nkv, bs):
    """rope_qkv_decode into a bf16 cache and rope_qkv_decode_fp8 into an fp8
    cache from the same inputs: the fp8 rows at pos are the reference
    quantization of the bf16 rows, q is the same, nothing else is touched.
    K head 0 of sequence 0 is all zero; the last K and V head rows of the
    last sequence carry a 2^15 x outlier (K only where that is another row
    than the zero row)."""
    maxlen = 32
    qkvd = (nq + 2 * nkv) * hd
    cosb, sinb = _rope_tables(maxlen, hd)
    torch.manual_seed(100 * hd + 10 * nq + bs)
    base = torch.randn(bs, qkvd)
    k0 = nq * hd
    base[0, k0:k0 + hd] = 0
    k_outlier = bs > 1 or nkv > 1  # else that row is the zero row
    if k_outlier:
        base[bs - 1, k0 + nkv * hd - hd + 5] = 2.0 ** 15  # last K head
    base[bs - 1, qkvd - hd + 7] = -(2.0 ** 15)  # last V head
    bias = torch.randn(qkvd)
    bias[k0:k0 + hd] = 0  # keeps the zero row zero
    bias = bias.to(torch.bfloat16).cuda()
    qkv_bf = base.to(torch.bfloat16).cuda()
    slabs = torch.stack([0.5 * base, 0.25 * base + torch.randn(bs, qkvd),
                         0.25 * base]).cuda()
    slabs[1, 0, k0:k0 + hd] = 0
    lens_sets = [[1], [maxlen]] if bs == 1 else [
        [(1, maxlen, 7, 20, 13)[i % 5] for i in range(bs)]]
    for lens, qkv, use_bias, rope in itertools.product(
            lens_sets, (qkv_bf, slabs), (False, True), (True, False)):
        cs = torch.tensor(lens, dtype=torch.int32, device="cuda")
        kc = torch.zeros(bs, maxlen, nkv, hd, dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
        k8, v8 = _filled(bs, maxlen, nkv, hd), _filled(bs, maxlen, nkv, hd)
        b = bias if use_bias else None
        q_ref = C.rope_qkv_decode(qkv, b, kc, vc, cs, cosb, sinb, nq, rope)
        q = C.rope_qkv_decode_fp8(qkv, b, k8.codes, k8.scale, v8.codes,
                                  v8.scale, cs, cosb, sinb, nq, rope)
        assert torch.equal(q, q_ref)
        seq = torch.arange(bs)
        pos = torch.tensor(lens) - 1
        what = f"append hd{hd} {nq}/{nkv} bs{bs} " \
               f"{'slab' if qkv.dim() == 3 else 'bf16'} bias={use_bias} rope={rope}"
        kq, ks = _check_cache(k8, kc.cpu()[seq, pos], seq, pos, what + " K")
        vq, vs = _check_cache(v8, vc.cpu()[seq, pos], seq, pos, what + " V")
        # the zero row: +-0 (RoPE of zeros can give -0, as in the bf16 cache)
        assert ks[0, 0] == 1.0 and int((kq[0, 0] & 0x7F).sum()) == 0
        outliers = [vq[bs - 1, nkv - 1]] + ([kq[bs - 1, nkv - 1]] if k_outlier else [])
        for got in outliers:
            assert (got & 0x7F).max() == 0x7E
            sub = ((got & 0x78) == 0) & ((got & 0x7F) != 0)
            assert int(sub.sum()) > hd // 8


# ---------------------------------------------------------------------------
# quantizing prefill store
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_prefill_store_bitwise(hd, nq, nkv, monkeypatch):
    """Packed lengths [12, 9, 5, 1] into maxlen 128; K and V are the views
    into the QKV projection the block hands over (token stride qkvd)."""
    lens = [12, 9, 5, 1]
    bs, maxlen, total = 4, 128, sum(lens)
    torch.manual_seed(hd + nkv)
    qkv = torch.randn(total, (nq + 2 * nkv) * hd)
    qkv[3, nq * hd:nq * hd + hd] = 0  # a zero K row
    qkv[20, -hd + 9] = 2.0 ** 15  # an outlier V row
    qkv = qkv.to(torch.bfloat16).cuda()
    _, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    k, v = k.reshape(total, nkv, hd), v.reshape(total, nkv, hd)
    assert not k.is_contiguous()
    cu = torch.tensor([0, 12, 21, 26, 27], dtype=torch.int32, device="cuda")
    pos = torch.cat([torch.arange(n) for n in lens])
    seq = torch.cat([torch.full((n,), i) for i, n in enumerate(lens)])
    k8, v8 = _filled(bs, maxlen, nkv, hd), _filled(bs, maxlen, nkv, hd)
    spy = []
    real = C.kv_store_fp8
    monkeypatch.delenv(KILL, raising=False)
    monkeypatch.setattr(C, "kv_store_fp8",
                        lambda *a: (spy.append(a), real(*a))[1])
    F.fp8_kv_store(k, v, k8, v8, cu, pos.cuda())
    assert len(spy) == 1 and spy[0][0].data_ptr() == k.data_ptr()  # no copy
    kq, ks = _check_cache(k8, k.cpu(), seq, pos, f"store hd{hd} nkv{nkv} K")
    _check_cache(v8, v.cpu(), seq, pos, f"store hd{hd} nkv{nkv} V")
    assert ks[3, 0] == 1.0 and int(kq[3, 0].sum()) == 0


# ---------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 8])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_every_v_code_decodes_exactly(hd, rep):
    """L = 1 and scales 1: the softmax weight is exactly 1, so the output is
    the decoded V row.  The V codes cycle through the 254 finite e4m3 codes
    (subnormals included), which pins the lane -> dim map of the PV read."""
    bs, nkv, maxlen = 4, 2, 8
    nq = nkv * rep
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    assert bs * nkv * hd >= 254
    v8 = codes[torch.arange(bs * nkv * hd) % 254].view(bs, nkv, hd)
    want = v8.view(torch.float8_e4m3fn).float()  # CPU decode
    assert torch.isfinite(want).all() and want.abs().max() == 448.0
    kc = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cuda")
    vc = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cuda")
    kc.scale.fill_(1.0)
    vc.scale.fill_(1.0)
    vc.codes.view(torch.uint8)[:, 0] = v8.cuda()
    torch.manual_seed(2)
    q = torch.randn(bs, nq, hd, device="cuda").to(torch.bfloat16)
    lens = torch.ones(bs, dtype=torch.int32, device="cuda")
    out = C.attn_decode_fp8(q, kc.codes, kc.scale, vc.codes, vc.scale, lens,
                            hd ** -0.5, 0)
    got = out.float().cpu().view(bs, nkv, rep, hd)
    bad = got != want[:, :, None, :]
    print("exact V decode hd", hd, "rep", rep, "mismatches", int(bad.sum()))
    assert int(bad.sum()) == 0


def _attn_case(bs, maxlen, nq, nkv, hd, seed):
    """Random bf16 K/V quantized by the reference; the scales are then
    overwritten by 2^((key % 16) - 8) for K and 2^(((key + 5) % 16) - 8) for
    V, so a mis-indexed scale cannot hide.  q is small enough that several
    keys share the softmax."""
    torch.manual_seed(seed)
    caches = []
    for shift in (0, 5):
        x = torch.randn(bs * maxlen * nkv, hd).to(torch.bfloat16)
        q8, _ = F.quantize_rows_e4m3_ref(x)
        key = torch.arange(maxlen)
        s = torch.pow(2.0, ((key + shift) % 16 - 8).float())
        caches.append(F.Fp8KVCache(
            q8.reshape(bs, maxlen, nkv, hd),
            s[None, None, :].expand(bs, nkv, maxlen).contiguous()))
    q = (torch.randn(bs, nq, hd) * 2.0 ** -13).to(torch.bfloat16)
    return q, caches[0], caches[1]


def _to_gpu(c):
    return F.Fp8KVCache(c.codes.cuda(), c.scale.cuda())


def _poison(c, lens, window):
    for b, L in enumerate(lens):
        lo = max(0, L - window) if window else 0
        c.codes.view(torch.uint8)[b, L:] = 0x7F
        c.codes.view(torch.uint8)[b, :lo] = 0x7F
        c.scale[b, :, L:] = float("nan")
        c.scale[b, :, :lo] = float("nan")


def _check_attn(q, kc, vc, lens, window, what):
    lens_t = torch.tensor(lens, dtype=torch.int32)
    scale = q.shape[-1] ** -0.5
    ref = F.attn_decode_ref(q.float(), kc.dequantize(), vc.dequantize(),
                            lens_t, scale, window=window)  # fp32, CPU
    out = F.attn_decode(q.cuda(), _to_gpu(kc), _to_gpu(vc), lens_t.cuda(),
                        scale, window=window)
    assert out.dtype == torch.bfloat16
    got = out.float().cpu()
    print(what, "max |err|", (got - ref).abs().max().item(), "max |ref|",
          ref.abs().max().item())
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    assert ref.abs().max() > 1
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


LENS8 = [1, 50, 64, 200, 255, 256, 257, 399]


@pytest.mark.parametrize("nq,nkv", [(8, 8), (8, 2), (8, 1), (4, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_attn_matches_fp32_reference(hd, nq, nkv, monkeypatch):
    """maxlen 400 in 8 splits, some of them empty.  Tolerance of
    test_attn_decode: the codes convert exactly and the scales apply in
    fp32, so the fp8 kernel adds no rounding the bf16 kernel lacks."""
    monkeypatch.delenv(KILL, raising=False)
    q, kc, vc = _attn_case(8, 400, nq, nkv, hd, seed=hd + nq + nkv)
    _check_attn(q, kc, vc, LENS8, None, f"attn fp8 hd{hd} {nq}/{nkv}")


def test_attn_no_split_epilogue(monkeypatch):
    """bs * nkv = 512: nsplit = 1, the no-workspace epilogue."""
    monkeypatch.delenv(KILL, raising=False)
    bs = 64
    lens = [1 + (37 * i) % 130 for i in range(bs)]
    assert min(lens) == 1 and max(lens) == 130
    q, kc, vc = _attn_case(bs, 130, 8, 8, 64, seed=9)
    _check_attn(q, kc, vc, lens, None, "attn fp8 nsplit 1")


@pytest.mark.parametrize("window,lens", [(100, [1, 99, 100, 101, 399]),
                                         (None, [1, 63, 65, 257])])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_attn_poisoned_outside(hd, window, lens, monkeypatch):
    """Every position outside [L - window, L) holds NaN codes and NaN
    scales: none of it may reach the output."""
    monkeypatch.delenv(KILL, raising=False)
    q, kc, vc = _attn_case(len(lens), 400, 8, 2, hd, seed=hd + len(lens))
    _poison(kc, lens, window)
    _poison(vc, lens, window)
    _check_attn(q, kc, vc, lens, window,
                f"attn fp8 poisoned hd{hd} window={window}")


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


def _gemma(seed=44):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("gemma").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=1, head_dim=256,
        vocab_size=256, intermediate_dim=512,
    )
    cfg.family = "gemma"
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init()
    with torch.no_grad():  # norm weights: 0.1 * randn, as in the gemma tests
        for t in m._params.values():
            if t.ndim == 1:
                t.copy_(0.1 * torch.randn_like(t))
    return cfg, m


def _prompts(device="cuda"):
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 256, (sum(LENS),), generator=g)
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    return toks.to(device), cu.to(device)


def _gconfig(kv, graph, weight=None):
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


def _kernel_vs_kill_switch(monkeypatch, m, what):
    """Prefill + 8 greedy steps.  Returns after checking: graph == eager
    tokens, kernels within 3e-2 of the references on the same fp8 caches
    (teacher-forced), step-0 logits bitwise those of kv_quant="none", and
    session + graph reuse on a second generate()."""
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv(KILL, raising=False)
    g = _gconfig("fp8_e4m3", True)
    out_hip, lg_hip = _generate_logged(monkeypatch, m, g)
    sess = m._gen_session[1]
    graph = sess.decoder.graph
    assert graph is not None
    assert isinstance(sess.kv_caches[0][0], F.Fp8KVCache)
    assert out_hip.gen_tokens.shape == (3, STEPS + 1)
    out_again, _ = _generate_logged(monkeypatch, m, g)
    assert m._gen_session[1] is sess and sess.decoder.graph is graph
    assert torch.equal(out_again.gen_tokens, out_hip.gen_tokens)

    m._gen_session = None  # fresh session for the failing-capture run
    monkeypatch.setenv("REALHF_AMD_FORCE_GRAPH_FAIL", "1")
    out_eager, _ = _generate_logged(monkeypatch, m, g)
    assert m._gen_session[1].decoder.graph is None
    assert torch.equal(out_hip.gen_tokens, out_eager.gen_tokens)
    monkeypatch.delenv("REALHF_AMD_FORCE_GRAPH_FAIL")

    monkeypatch.setenv(KILL, "1")
    out_ref, lg_ref = _generate_logged(monkeypatch, m, g,
                                       forced=out_hip.gen_tokens)
    assert m._gen_session[1].decoder.graph is None  # the reference is eager
    assert isinstance(m._gen_session[1].kv_caches[0][0], F.Fp8KVCache)
    monkeypatch.delenv(KILL)
    assert torch.equal(out_ref.gen_tokens, out_hip.gen_tokens)
    print(what, "fp8 KV kernels vs references: max |diff|",
          (lg_hip - lg_ref).abs().max().item(), "max |logit|",
          lg_ref.abs().max().item())
    assert lg_ref.abs().max() > 0.1
    torch.testing.assert_close(lg_hip, lg_ref, atol=3e-2, rtol=3e-2)

    _, lg_none = _generate_logged(monkeypatch, m, _gconfig("none", True),
                                  forced=out_hip.gen_tokens)
    assert torch.equal(lg_hip[0], lg_none[0])  # prefill is unquantized
    assert (lg_hip[1:] - lg_none[1:]).abs().max() > 0


def test_model_fp8_kv_matches_kill_switch(monkeypatch):
    _, m = _llama()
    _kernel_vs_kill_switch(monkeypatch, m, "llama")


def test_gemma_fp8_kv_matches_kill_switch(monkeypatch):
    """hd 256, gemma_rms, GeGLU."""
    _, m = _gemma()
    _kernel_vs_kill_switch(monkeypatch, m, "gemma")


def test_model_dispatch(monkeypatch):
    """kv_quant="none" (and the unset default) calls exactly the entry
    points the parent commit called and none of the new ones; "fp8_e4m3"
    moves the append and the attention of every layer and decode step, and
    the prefill store of every layer, to the fp8 entry points."""
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv(WENV, raising=False)
    monkeypatch.delenv(KILL, raising=False)
    cfg, m = _llama(seed=46)
    old = ("rope_qkv_decode", "attn_decode", "skinny_gemm", "skinny_gemm_nc")
    new = ("rope_qkv_decode_fp8", "attn_decode_fp8", "kv_store_fp8")
    wq = ("skinny_gemm_fp8", "skinny_gemm_fp8_nc", "quantize_rows_e4m3_")
    seen = {n: [] for n in old + new + wq}

    def spy(name):
        real = getattr(C, name)

        def f(*a):
            seen[name].append(a)
            return real(*a)

        monkeypatch.setattr(C, name, f)

    for n in seen:
        spy(n)
    L = cfg.n_layers

    def run(kv, weight=None):
        for v in seen.values():
            v.clear()
        m._gen_session = None
        return _generate_logged(monkeypatch, m, _gconfig(kv, False, weight))[0]

    outs = {}
    for kv in (None, "none"):
        outs[kv] = run(kv)
        assert len(seen["rope_qkv_decode"]) == STEPS * L
        assert len(seen["attn_decode"]) == STEPS * L
        assert len(seen["skinny_gemm_nc"]) == STEPS * 3 * L
        assert len(seen["skinny_gemm"]) == STEPS * (L + 1)
        for n in new + wq:
            assert not seen[n], n
        assert isinstance(m._gen_session[1].kv_caches[0][0], torch.Tensor)
    assert torch.equal(outs[None].gen_logprobs, outs["none"].gen_logprobs)

    def check_fp8_kv():
        assert len(seen["rope_qkv_decode_fp8"]) == STEPS * L
        assert len(seen["attn_decode_fp8"]) == STEPS * L
        assert len(seen["kv_store_fp8"]) == L
        assert not seen["rope_qkv_decode"] and not seen["attn_decode"]

    run("fp8_e4m3")
    check_fp8_kv()
    assert len(seen["skinny_gemm_nc"]) == STEPS * 3 * L  # weights stay bf16
    for n in wq:
        assert not seen[n], n
    # the environment variable alone selects it, too
    monkeypatch.setenv(ENV, "fp8_e4m3")
    run(None)
    check_fp8_kv()
    monkeypatch.delenv(ENV)
    # with weight_quant both sets of entry points run
    run("fp8_e4m3", "fp8_e4m3")
    check_fp8_kv()
    assert len(seen["skinny_gemm_fp8_nc"]) == STEPS * 3 * L
    assert len(seen["skinny_gemm_fp8"]) == STEPS * L
    assert len(seen["quantize_rows_e4m3_"]) == 4 * L
    assert not seen["skinny_gemm_nc"]


def _teacher_forced(m, forced, fp8_kv):
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
        lg = m(packed_input_ids=forced[:, t], kv_caches=kv,
               cache_seqlens=seqlens, decode=True)
        lp = torch.log_softmax(lg.float(), -1)
        logps.append(lp.gather(-1, forced[:, t + 1].unsqueeze(-1)).squeeze(-1))
    return torch.stack(logps, 1).cpu()


def test_quantization_error_no_worse_than_fp32_reference(monkeypatch):
    """Mean |log-prob difference| of the forced tokens between fp8-KV and
    bf16-KV decode on the kernels, against the same quantity for an fp32 CPU
    copy of the model with and without the reference fp8 cache.  Both see
    the same quantization rule; the kernel path adds only bf16 rounding, so
    e_kernel <= 2 * e_ref + 1e-3, the rule of
    test_fp8_decode_gpu.test_quantization_error_no_worse_than_fp32_reference."""
    from realhf_amd.models.real_model import ReaLModel

    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv(KILL, raising=False)
    cfg, m = _llama(seed=47)
    out, _ = _generate_logged(monkeypatch, m, _gconfig("none", False))
    forced = out.gen_tokens  # [bs, STEPS + 1], sampled by the bf16 model
    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
        lp_bf16 = _teacher_forced(m, forced, False)
        lp_fp8 = _teacher_forced(m, forced, True)
        lp_32 = _teacher_forced(m32, forced, False)
        lp_32_fp8 = _teacher_forced(m32, forced, True)
    e_kernel = (lp_fp8 - lp_bf16).abs().mean().item()
    e_ref = (lp_32_fp8 - lp_32).abs().mean().item()
    print(f"mean |dlogp| fp8 KV vs unquantized KV: kernel path {e_kernel:.4e}, "
          f"fp32 CPU reference {e_ref:.4e}")
    assert e_ref > 0 and e_kernel > 0
    assert e_kernel <= 2 * e_ref + 1e-3
