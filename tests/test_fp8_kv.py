"""FP8 (e4m3) KV cache on the CPU: kv_quant resolution and downgrade rules,
the session key and cache size, the torch references of the quantizing
append / prefill store and of decode attention over (codes, scale), and a
tiny fp32 llama generating through them."""
import types

import pytest
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.api.model import GenerationHyperparameters
from realhf_amd.models import generation as genmod
from realhf_amd.models.generation import generate
from realhf_amd.models.real_model import ReaLModel
from realhf_amd.ops import functional as F

ENV = "REALHF_AMD_GEN_KV_QUANT"


def _u8(t):
    return t.view(torch.uint8)


# ---------------------------------------------------------------------------
# kv_quant resolution
# ---------------------------------------------------------------------------
def _g(**kw):
    kw.setdefault("max_new_tokens", 4)
    return GenerationHyperparameters(greedy=True, use_hip_graph=False, **kw)


def test_resolution_field_env_and_bad_values(monkeypatch):
    assert GenerationHyperparameters().kv_quant is None
    monkeypatch.delenv(ENV, raising=False)
    assert genmod.resolve_kv_quant(_g()) == "none"
    assert genmod.resolve_kv_quant(_g(kv_quant="none")) == "none"
    assert genmod.resolve_kv_quant(_g(kv_quant="fp8_e4m3")) == "fp8_e4m3"
    monkeypatch.setenv(ENV, "fp8_e4m3")
    assert genmod.resolve_kv_quant(_g()) == "fp8_e4m3"  # read at call time
    assert genmod.resolve_kv_quant(_g(kv_quant="none")) == "none"  # field wins
    monkeypatch.setenv(ENV, "none")
    assert genmod.resolve_kv_quant(_g(kv_quant="fp8_e4m3")) == "fp8_e4m3"
    monkeypatch.setenv(ENV, "")
    assert genmod.resolve_kv_quant(_g()) == "none"
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(ValueError, match="kv_quant"):
        genmod.resolve_kv_quant(_g())
    monkeypatch.delenv(ENV)
    with pytest.raises(ValueError, match="kv_quant"):
        genmod.resolve_kv_quant(_g(kv_quant="int8"))


def _tiny_llama(seed=0, dtype=torch.bfloat16, n_layers=2):
    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=n_layers, hidden_dim=128, n_heads=2, n_kv_heads=2, head_dim=64,
        intermediate_dim=256, vocab_size=128,
    )
    cfg.family = "llama"
    m = ReaLModel(cfg, device="cpu", dtype=dtype)
    torch.manual_seed(seed)
    m.random_init(std=0.05)
    return cfg, m


def _prompts():
    toks = torch.tensor([5, 9, 33, 7, 101, 64, 12, 3, 88], dtype=torch.long)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32)
    return toks, cu


def test_bad_value_raises_in_generate(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _, m = _tiny_llama()
    with pytest.raises(ValueError, match="kv_quant"):
        generate(m, *_prompts(), _g(kv_quant="e5m2"))
    monkeypatch.setenv(ENV, "yes")
    with pytest.raises(ValueError, match="kv_quant"):
        generate(m, *_prompts(), _g())


def _stub(**kw):
    """What kv_quant_blocker reads of a model."""
    cfg = types.SimpleNamespace(qk_layernorm=False, head_dim=128)
    d = dict(config=cfg, lora_flat=None, dtype=torch.bfloat16, pp_size=1,
             flat_param=types.SimpleNamespace(is_cuda=True))
    for k, v in kw.items():
        if k in ("qk_layernorm", "head_dim"):
            setattr(cfg, k, v)
        else:
            d[k] = v
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("kw,env,word", [
    (dict(lora_flat=object()), None, "LoRA"),
    (dict(qk_layernorm=True), None, "qk_layernorm"),
    (dict(head_dim=96), None, "head_dim 96"),
    (dict(dtype=torch.float32), None, "float32"),
    (dict(), "REALHF_AMD_NO_FUSED_DECODE", "NO_FUSED_DECODE"),
    (dict(pp_size=2), None, "pp > 1"),
])
def test_each_blocker_downgrades_with_one_warning(monkeypatch, kw, env, word):
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv("REALHF_AMD_NO_FUSED_DECODE", raising=False)
    assert genmod.kv_quant_blocker(_stub()) is None
    if env:
        monkeypatch.setenv(env, "1")
    m = _stub(**kw)
    assert word in genmod.kv_quant_blocker(m)
    warned = []
    monkeypatch.setattr(genmod.logger, "warning",
                        lambda *a, **k: warned.append(a))
    for _ in range(3):
        assert genmod.effective_kv_quant(m, _g(kv_quant="fp8_e4m3")) == "none"
    assert len(warned) == 1 and word in (warned[0][0] % warned[0][1:])
    # not asked for: nothing to warn about
    assert genmod.effective_kv_quant(_stub(**kw), _g(kv_quant="none")) == "none"
    assert len(warned) == 1


def test_cpu_model_of_any_dtype_is_not_blocked(monkeypatch):
    monkeypatch.delenv("REALHF_AMD_NO_FUSED_DECODE", raising=False)
    for dt in (torch.float32, torch.bfloat16):
        _, m = _tiny_llama(dtype=dt, n_layers=1)
        assert genmod.kv_quant_blocker(m) is None
    m.attach_lora(dim=4)
    assert "LoRA" in genmod.kv_quant_blocker(m)


def test_downgraded_generate_uses_dense_caches(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.setenv("REALHF_AMD_NO_FUSED_DECODE", "1")
    _, m = _tiny_llama(n_layers=1)
    warned = []
    monkeypatch.setattr(genmod.logger, "warning",
                        lambda *a, **k: warned.append(a))
    for _ in range(2):
        out = generate(m, *_prompts(), _g(kv_quant="fp8_e4m3"))
    assert out.gen_tokens.shape == (2, 4)
    kc, vc = m._gen_session[1].kv_caches[0]
    assert isinstance(kc, torch.Tensor) and kc.dtype == torch.bfloat16
    assert len(warned) == 1


def test_session_key_and_cache_bytes(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv("REALHF_AMD_NO_FP8_KV", raising=False)
    cfg, m = _tiny_llama()
    toks, cu = _prompts()
    generate(m, toks, cu, _g(kv_quant="none"))
    key_none, sess_none = m._gen_session
    generate(m, toks, cu, _g())
    assert m._gen_session[1] is sess_none  # unset == none: session reused
    generate(m, toks, cu, _g(kv_quant="fp8_e4m3"))
    key_fp8, sess_fp8 = m._gen_session
    assert key_fp8 != key_none and sess_fp8 is not sess_none
    generate(m, toks, cu, _g(kv_quant="fp8_e4m3"))
    assert m._gen_session[1] is sess_fp8
    # the kill switch state is in the key
    monkeypatch.setenv("REALHF_AMD_NO_FP8_KV", "1")
    generate(m, toks, cu, _g(kv_quant="fp8_e4m3"))
    assert m._gen_session[0] != key_fp8
    monkeypatch.delenv("REALHF_AMD_NO_FP8_KV")
    # ... and so is weight_quant, independently
    generate(m, toks, cu, _g(kv_quant="fp8_e4m3", weight_quant="fp8_e4m3"))
    key_both, sess_both = m._gen_session
    assert key_both not in (key_fp8, key_none) and sess_both.fp8 is not None

    bs, cache_len = 2, 128  # 5 + 4 tokens, bucketed to 128
    caches = sess_both.kv_caches
    assert len(caches) == cfg.n_layers and all(len(p) == 2 for p in caches)
    total = 0
    for pair in caches:
        for c in pair:
            assert isinstance(c, F.Fp8KVCache)
            assert c.shape == (bs, cache_len, cfg.n_kv_heads, cfg.head_dim)
            assert c.codes.dtype == torch.float8_e4m3fn
            assert c.scale.shape == (bs, cfg.n_kv_heads, cache_len)
            for t in (c.codes, c.scale):
                total += t.numel() * t.element_size()
    assert total == (2 * cfg.n_layers * bs * cache_len * cfg.n_kv_heads
                     * (cfg.head_dim + 4))
    assert total == sum(c.nbytes() for pair in caches for c in pair)


# ---------------------------------------------------------------------------
# reference append and prefill store
# ---------------------------------------------------------------------------
def _rows(n, nkv, hd, seed):
    torch.manual_seed(seed)
    x = torch.randn(n, nkv, hd)
    x[0, 0] = 0  # an all-zero head row
    x[-1, -1, 3] = 2.0 ** 15  # outlier: the rest of the row goes subnormal
    return x


def _fresh(bs, maxlen, nkv, hd):
    c = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cpu")
    _u8(c.codes).fill_(0x55)
    c.scale.fill_(-1.0)
    return c


def _check_rows(cache, x, seq, pos):
    """cache rows at (seq, pos) == quantize_rows_e4m3_ref of the bf16 rows;
    everything else still holds the fill pattern."""
    n, nkv, hd = x.shape
    q, s = F.quantize_rows_e4m3_ref(x.to(torch.bfloat16).reshape(-1, hd))
    q, s = _u8(q).reshape(n, nkv, hd), s.reshape(n, nkv)
    touched = torch.zeros(cache.shape[:2], dtype=torch.bool)
    for i in range(n):
        b, p = int(seq[i]), int(pos[i])
        assert torch.equal(_u8(cache.codes)[b, p], q[i])
        assert torch.equal(cache.scale[b, :, p].view(torch.int32),
                           s[i].view(torch.int32))
        touched[b, p] = True
    assert (_u8(cache.codes)[~touched] == 0x55).all()
    assert (cache.scale.transpose(1, 2)[~touched] == -1.0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ref_append(dtype):
    bs, maxlen, nkv, hd = 3, 16, 2, 64
    k, v = _rows(bs, nkv, hd, 1).to(dtype), _rows(bs, nkv, hd, 2).to(dtype)
    kc, vc = _fresh(bs, maxlen, nkv, hd), _fresh(bs, maxlen, nkv, hd)
    lens = torch.tensor([1, 7, maxlen], dtype=torch.int32)
    F.fp8_kv_append_ref(k, v, kc, vc, lens)
    _check_rows(kc, k.float(), torch.arange(bs), lens - 1)
    _check_rows(vc, v.float(), torch.arange(bs), lens - 1)
    # the all-zero row: scale 1, codes 0
    assert kc.scale[0, 0, 0] == 1.0 and int(_u8(kc.codes)[0, 0, 0].sum()) == 0
    # the outlier row: 448 and subnormal codes
    row = _u8(kc.codes)[2, maxlen - 1, 1]
    assert row[3] == 0x7E
    assert int((((row & 0x78) == 0) & ((row & 0x7F) != 0)).sum()) > hd // 4


def test_ref_store_packed():
    lens = [12, 9, 5, 1]
    bs, maxlen, nkv, hd = 4, 32, 2, 64
    total = sum(lens)
    k, v = _rows(total, nkv, hd, 3), _rows(total, nkv, hd, 4)
    cu = torch.tensor([0, 12, 21, 26, 27], dtype=torch.int32)
    pos = torch.cat([torch.arange(n) for n in lens])
    seq = torch.cat([torch.full((n,), i) for i, n in enumerate(lens)])
    kc, vc = _fresh(bs, maxlen, nkv, hd), _fresh(bs, maxlen, nkv, hd)
    F.fp8_kv_store(k, v, kc, vc, cu, pos)  # CPU: the reference
    _check_rows(kc, k, seq, pos)
    _check_rows(vc, v, seq, pos)
    assert kc.scale[0, 0, 0] == 1.0 and int(_u8(kc.codes)[0, 0, 0].sum()) == 0


# ---------------------------------------------------------------------------
# reference decode attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("window", [None, 20])
def test_ref_attention_equals_dequantized(nq, nkv, window):
    torch.manual_seed(7)
    bs, maxlen, hd = 4, 48, 64
    caches = []
    for _ in range(2):
        x = torch.randn(bs * maxlen, nkv, hd).to(torch.bfloat16)
        q8, s = F.quantize_rows_e4m3_ref(x.reshape(-1, hd))
        caches.append(F.Fp8KVCache(
            q8.reshape(bs, maxlen, nkv, hd),
            s.reshape(bs, maxlen, nkv).transpose(1, 2).contiguous()))
    kc, vc = caches
    deq = kc.dequantize()
    assert deq.shape == (bs, maxlen, nkv, hd) and deq.dtype == torch.float32
    assert torch.equal(deq[1, 5, nkv - 1],
                       kc.codes[1, 5, nkv - 1].float() * kc.scale[1, nkv - 1, 5])
    q = torch.randn(bs, nq, hd)
    lens = torch.tensor([1, 19, 21, maxlen], dtype=torch.int32)
    want = F.attn_decode_ref(q, deq, vc.dequantize(), lens, 0.2, window=window)
    got = F.attn_decode_fp8_ref(q, kc, vc, lens, 0.2, window=window)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-6)
    # the dispatcher takes the pair, and bf16 q comes back as bf16
    got2 = F.attn_decode(q, kc, vc, lens, 0.2, window=window)
    assert torch.equal(got2, got)
    got_bf = F.attn_decode(q.to(torch.bfloat16), kc, vc, lens, 0.2, window=window)
    assert got_bf.dtype == torch.bfloat16
    # outside [lo, L) nothing is read: poison it
    for b in range(bs):
        L = int(lens[b])
        lo = max(0, L - window) if window else 0
        for c in (kc, vc):
            _u8(c.codes)[b, L:] = 0x7F
            _u8(c.codes)[b, :lo] = 0x7F
            c.scale[b, :, L:] = float("nan")
            c.scale[b, :, :lo] = float("nan")
    got3 = F.attn_decode_fp8_ref(q, kc, vc, lens, 0.2, window=window)
    assert torch.equal(got3, got)


# ---------------------------------------------------------------------------
# tiny fp32 llama on the CPU: 2 layers, hidden 256, intermediate 512, hd 128
# ---------------------------------------------------------------------------
def _llama32(seed=44):
    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=2, head_dim=128,
        vocab_size=256, intermediate_dim=512,
    )
    cfg.family = "llama"
    cfg.dtype = "float32"
    torch.manual_seed(seed)
    m = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    m.random_init(std=0.05)
    return cfg, m


def _generate_logged(monkeypatch, m, gconfig, toks, cu):
    seen = []
    real = genmod._sample_from_logits

    def spy(logits, *a, **kw):
        seen.append(logits.clone())
        return real(logits, *a, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(genmod, "_sample_from_logits", spy)
        out = generate(m, toks, cu, gconfig)
    return out, torch.stack(seen)


def test_fp32_cpu_llama_generates(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _llama32()
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 256, (26,), generator=g)
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32)
    calls = {"append": 0, "store": 0, "attn": 0}
    for name, key in (("fp8_kv_append_ref", "append"),
                      ("fp8_kv_store_ref", "store"),
                      ("attn_decode_fp8_ref", "attn")):
        real = getattr(F, name)

        def spy(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(F, name, spy)
    out_ref, lg_ref = _generate_logged(monkeypatch, m, _g(kv_quant="none",
                                                          max_new_tokens=6),
                                       toks, cu)
    assert calls == {"append": 0, "store": 0, "attn": 0}
    out, lg = _generate_logged(monkeypatch, m, _g(kv_quant="fp8_e4m3",
                                                  max_new_tokens=6), toks, cu)
    assert out.gen_tokens.shape == (3, 6) and lg.shape == lg_ref.shape
    L = cfg.n_layers
    assert calls == {"append": 5 * L, "store": L, "attn": 5 * L}
    # prefill attention runs on the fresh, unquantized K/V
    assert torch.equal(lg[0], lg_ref[0])
    assert torch.equal(out.gen_tokens[:, 0], out_ref.gen_tokens[:, 0])
    d = (lg[1:] - lg_ref[1:]).abs().max().item()
    print("decode logits, fp8 KV vs fp32 KV: max |diff|", d)
    assert d > 0 and torch.isfinite(lg).all()
    # the prompt rows of layer 0 are the reference quantization of a bf16 K
    kc, vc = m._gen_session[1].kv_caches[0]
    assert isinstance(kc, F.Fp8KVCache)
    row = kc.codes[1, 3, 0].float()
    assert row.abs().max() == 448.0 and kc.scale[1, 0, 3] > 0
    assert int(_u8(kc.codes)[0, 12 + 6:].sum()) == 0  # never written: zeros
    # composes with weight_quant on a bf16 model (fp32 models downgrade that)
    _, mb = _tiny_llama()
    out_b = generate(mb, *_prompts(), _g(kv_quant="fp8_e4m3",
                                         weight_quant="fp8_e4m3"))
    assert out_b.gen_tokens.shape == (2, 4)
    assert mb._gen_session[1].fp8 is not None
    assert isinstance(mb._gen_session[1].kv_caches[0][0], F.Fp8KVCache)
