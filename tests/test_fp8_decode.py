"""FP8 weight-only decode on the CPU: the reference quantizer's definition
and generate()'s weight_quant plumbing (field, environment variable, session
key, in-place refresh) on a tiny bf16 llama, where every quantized
projection goes through fp8_linear_ref."""
import pytest
import torch

import realhf_amd.models.hf as hf_reg
from realhf_amd.api.model import GenerationHyperparameters
from realhf_amd.models import generation as genmod
from realhf_amd.models.generation import generate
from realhf_amd.models.real_model import ReaLModel
from realhf_amd.ops import functional as F

ENV = "REALHF_AMD_GEN_WEIGHT_QUANT"


# ---------------------------------------------------------------------------
# reference quantizer
# ---------------------------------------------------------------------------
def _weights(seed=0):
    torch.manual_seed(seed)
    w = (0.02 * torch.randn(6, 256)).to(torch.bfloat16)
    w[2] = 0  # all-zero row
    w[4, 17] = 640.0  # 2^15 x outlier: most of the row lands in subnormals
    return w


def test_ref_scale_is_amax_over_448():
    w = _weights()
    q, scale = F.quantize_rows_e4m3_ref(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (6,)
    amax = w.float().abs().amax(dim=1)
    want = amax / 448.0
    want[2] = 1.0
    assert torch.equal(scale, want)
    # the row maximum lands on +-448 exactly
    qa = q.float().abs().amax(dim=1)
    assert torch.equal(qa[[0, 1, 3, 4, 5]], torch.full((5,), 448.0))


def test_ref_zero_row():
    q, scale = F.quantize_rows_e4m3_ref(_weights())
    assert scale[2] == 1.0
    assert torch.equal(q[2].view(torch.uint8), torch.zeros(256, dtype=torch.uint8))


def test_ref_no_nan_codes():
    torch.manual_seed(3)
    w = torch.cat([_weights(), (5.0 * torch.randn(64, 256)).to(torch.bfloat16)])
    q, _ = F.quantize_rows_e4m3_ref(w)
    codes = q.view(torch.uint8) & 0x7F
    assert int((codes == 0x7F).sum()) == 0
    assert torch.isfinite(q.float()).all()


def test_ref_dequantization_error():
    """Elements at or above amax / 2^6 of their row are e4m3 normals after
    scaling (448 / 64 = 7 >= 2^-6), so they carry half an ulp of a 3-bit
    mantissa: 2^-4 relative."""
    torch.manual_seed(4)
    w = torch.cat([_weights(), torch.randn(32, 512)[:, :256].to(torch.bfloat16)])
    q, scale = F.quantize_rows_e4m3_ref(w)
    wf = w.float()
    deq = q.float() * scale[:, None]
    amax = wf.abs().amax(dim=1, keepdim=True)
    big = (wf.abs() >= amax / 64) & (wf != 0)
    rel = ((deq - wf).abs() / wf.abs().clamp_min(1e-30))[big]
    assert big.sum() > 1000
    print("max relative dequantization error", rel.max().item())
    assert rel.max() <= 2.0 ** -4


def test_fp8_linear_ref():
    torch.manual_seed(5)
    w = _weights()
    q, scale = F.quantize_rows_e4m3_ref(w)
    x = torch.randn(3, 256).to(torch.bfloat16)
    r = torch.randn(3, 6).to(torch.bfloat16)
    want = x.float() @ (q.float() * scale[:, None]).t()
    assert torch.equal(F.fp8_linear_ref(x.float(), q, scale), want)
    got = F.fp8_linear_ref(x, q, scale, residual=r)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, (want + r.float()).to(torch.bfloat16))


# ---------------------------------------------------------------------------
# generate() on a tiny CPU llama
# ---------------------------------------------------------------------------
def _tiny_llama(seed=0):
    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=2, hidden_dim=128, n_heads=2, n_kv_heads=2, head_dim=64,
        intermediate_dim=256, vocab_size=128,
    )
    cfg.family = "llama"
    m = ReaLModel(cfg, device="cpu", dtype=torch.bfloat16)
    torch.manual_seed(seed)
    m.random_init(std=0.05)
    return cfg, m


def _prompts():
    toks = torch.tensor([5, 9, 33, 7, 101, 64, 12, 3, 88], dtype=torch.long)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32)
    return toks, cu


def _g(**kw):
    kw.setdefault("max_new_tokens", 4)
    return GenerationHyperparameters(greedy=True, use_hip_graph=False, **kw)


@pytest.fixture
def ref_calls(monkeypatch):
    calls = []
    real = F.fp8_linear_ref

    def spy(x, q, scale, residual=None):
        calls.append((q, scale))
        return real(x, q, scale, residual)

    monkeypatch.setattr(F, "fp8_linear_ref", spy)
    return calls


def test_generate_fp8_goes_through_ref(ref_calls, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    cfg, m = _tiny_llama()
    toks, cu = _prompts()
    out = generate(m, toks, cu, _g(weight_quant="fp8_e4m3"))
    assert out.gen_tokens.shape == (2, 4)
    # 3 decode steps x 2 layers x (qkv, wo, gate/up, down); prefill is bf16
    assert len(ref_calls) == 3 * cfg.n_layers * 4
    fp8 = m._gen_session[1].fp8
    owned = {q.data_ptr() for d in fp8.pairs for q, _ in d.values()}
    assert {q.data_ptr() for q, _ in ref_calls} == owned
    assert all(set(d) == {"qkv", "wo", "gu", "down"} for d in fp8.pairs)
    # the pairs are the reference quantization of the current weights
    blk = fp8.blocks[0]
    q, s = fp8.pairs[0]["qkv"]
    qr, sr = F.quantize_rows_e4m3_ref(blk.decode_weights()["qkv"])
    assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8))
    assert torch.equal(s, sr)
    # nothing stays installed after the call: a bare decode step is bf16
    assert all(b.fp8 == {} for b in fp8.blocks)

    ref_calls.clear()
    out_bf16 = generate(m, toks, cu, _g(weight_quant="none"))
    assert not ref_calls
    assert m._gen_session[1].fp8 is None
    assert out_bf16.gen_tokens.shape == (2, 4)


def test_unknown_weight_quant_raises(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _, m = _tiny_llama()
    toks, cu = _prompts()
    with pytest.raises(ValueError, match="weight_quant"):
        generate(m, toks, cu, _g(weight_quant="int4"))
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(ValueError, match="weight_quant"):
        generate(m, toks, cu, _g())


def test_env_and_field_precedence(ref_calls, monkeypatch):
    _, m = _tiny_llama()
    toks, cu = _prompts()
    assert GenerationHyperparameters().weight_quant is None
    monkeypatch.delenv(ENV, raising=False)
    generate(m, toks, cu, _g())
    assert not ref_calls  # default: none
    monkeypatch.setenv(ENV, "fp8_e4m3")
    generate(m, toks, cu, _g())
    assert ref_calls  # field None: the environment decides, at call time
    ref_calls.clear()
    generate(m, toks, cu, _g(weight_quant="none"))
    assert not ref_calls  # the field wins
    monkeypatch.setenv(ENV, "none")
    generate(m, toks, cu, _g(weight_quant="fp8_e4m3"))
    assert ref_calls


def test_session_key_changes_with_mode(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _, m = _tiny_llama()
    toks, cu = _prompts()
    generate(m, toks, cu, _g(weight_quant="none"))
    key_none, sess_none = m._gen_session
    generate(m, toks, cu, _g(weight_quant="none"))
    assert m._gen_session[1] is sess_none  # same mode: session reused
    generate(m, toks, cu, _g(weight_quant="fp8_e4m3"))
    key_fp8, sess_fp8 = m._gen_session
    assert key_fp8 != key_none and sess_fp8 is not sess_none
    assert "fp8_e4m3" in key_fp8 and "none" in key_none
    generate(m, toks, cu, _g(weight_quant="fp8_e4m3"))
    assert m._gen_session[1] is sess_fp8


def test_refresh_in_place_after_flat_param_change(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _, m = _tiny_llama()
    toks, cu = _prompts()
    g = _g(weight_quant="fp8_e4m3")
    generate(m, toks, cu, g)
    fp8 = m._gen_session[1].fp8
    addrs = [(k, q.data_ptr(), s.data_ptr())
             for d in fp8.pairs for k, (q, s) in d.items()]
    before = [(q.view(torch.uint8).clone(), s.clone())
              for d in fp8.pairs for q, s in d.values()]
    with torch.no_grad():  # what an optimizer step does: in place, no rebind
        m.flat_param.mul_(1.5)
        m._params["1.mlp.down.weight"][3, 5] = 9.0
    generate(m, toks, cu, g)
    assert m._gen_session[1].fp8 is fp8
    assert addrs == [(k, q.data_ptr(), s.data_ptr())
                     for d in fp8.pairs for k, (q, s) in d.items()]
    after = [(q.view(torch.uint8), s) for d in fp8.pairs for q, s in d.values()]
    # every scale follows the 1.5x; the poked row is requantized
    for (_, s0), (_, s1) in zip(before, after):
        assert not torch.equal(s0, s1)
    for blk, d in zip(fp8.blocks, fp8.pairs):
        ws = blk.decode_weights()
        for k, (q, s) in d.items():
            qr, sr = F.quantize_rows_e4m3_ref(ws[k])
            assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8)), k
            assert torch.equal(s, sr), k
    q_down, s_down = fp8.pairs[0]["down"]
    assert s_down[3] == 9.0 / 448.0


def test_blockers_ignore_quant_with_one_warning(monkeypatch, ref_calls):
    """An fp32 model cannot use the fused decode block: the request is
    ignored and decode stays on the unquantized weights."""
    monkeypatch.delenv(ENV, raising=False)
    cfg = hf_reg.get_family("llama").make_test_config(
        n_layers=1, hidden_dim=128, n_heads=2, n_kv_heads=2, head_dim=64,
        intermediate_dim=256, vocab_size=128,
    )
    cfg.family = "llama"
    m = ReaLModel(cfg, device="cpu", dtype=torch.float32)
    torch.manual_seed(1)
    m.random_init()
    assert "bfloat16" in genmod.weight_quant_blocker(m)
    warned = []
    monkeypatch.setattr(genmod.logger, "warning",
                        lambda *a, **kw: warned.append(a))
    toks, cu = _prompts()
    for _ in range(2):
        generate(m, toks, cu, _g(weight_quant="fp8_e4m3"))
    assert not ref_calls and m._gen_session[1].fp8 is None
    assert len(warned) == 1

    _, mb = _tiny_llama()
    assert genmod.weight_quant_blocker(mb) is None
    monkeypatch.setenv("REALHF_AMD_NO_FUSED_DECODE", "1")
    assert "NO_FUSED_DECODE" in genmod.weight_quant_blocker(mb)
    monkeypatch.delenv("REALHF_AMD_NO_FUSED_DECODE")
    mb.attach_lora(dim=4)
    assert "LoRA" in genmod.weight_quant_blocker(mb)
