"""MoE decode from FP8 expert weights: the routed kernels against fp64, the k
mapping code by code, a tiny mixtral through generate(), quantization error."""
import collections
import math

import pytest
import torch

from test_fp8_decode_gpu import _prompts, _teacher_forced, _u8
from test_moe_decode_gpu import _generate, _mixtral, _routing
import realhf_amd._C as C
from realhf_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

KILL = "REALHF_AMD_NO_FP8_MOE"


@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("E,k", [(4, 2), (16, 8)])
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("H,I", [(256, 64), (256, 192), (1088, 1344)])
def test_expert_path_matches_fp64(H, I, M, E, k, kind):
    torch.manual_seed(0)
    idx, wts = _routing(kind, M, E, k)
    idle = torch.ones(E, dtype=torch.bool, device="cuda")
    idle[idx.long().flatten()] = False
    fp8 = []
    for n, kk in ((I, H), (I, H), (H, I)):
        # padded expert stride; rows scaled by 0.25 .. 4 (log-uniform: the
        # geometric mean stays 1, the scale the bf16 test's bound is set for)
        w = torch.empty(E, n * kk + 16, device="cuda", dtype=torch.bfloat16)
        w = w[:, :n * kk].view(E, n, kk)
        w.copy_(torch.randn(E, n, kk, device="cuda") / math.sqrt(kk)
                * 2 ** (4 * torch.rand(E, n, 1, device="cuda") - 2))
        q, s = ops.quantize_rows_e4m3(w)
        for e in range(E):  # the definition: the reference on the CPU
            q_ref, s_ref = ops.quantize_rows_e4m3_ref(w[e].cpu())
            assert torch.equal(s[e].cpu(), s_ref)
            assert torch.equal(_u8(q[e]), _u8(q_ref))
        q.view(torch.uint8)[idle] = 0x7F  # an idle expert contributes nothing
        s[idle] = float("nan")
        fp8.append((q, s))
    h = torch.randn(M, H, device="cuda").bfloat16()
    res = torch.randn(M, H, device="cuda").bfloat16()

    def run():  # every row consumed must have been written: NaN buffers
        act = torch.full((k, M, I), float("nan"), device="cuda",
                         dtype=torch.bfloat16)
        ws = torch.full((ops.moe_down_splitk(I) * k * 16 * H,), float("nan"),
                        device="cuda")
        return ops.moe_experts_decode(h, idx, wts, None, None, None,
                                      residual=res, act=act, ws=ws, fp8=fp8)

    out = run()
    assert out.shape == (M, H) and torch.isfinite(out).all()
    assert torch.equal(out, run())  # bitwise reproducible
    ref = ops.moe_decode_ref(
        h.double(), None, *(q.double() * s.double()[..., None] for q, s in fp8),
        k, False, residual=res.double(), routing=(idx.long(), wts.double()))
    torch.testing.assert_close(out.double(), ref, atol=3e-2, rtol=3e-2)


def test_every_code_decodes_exactly():
    """One-hot rows over every k of K = 128, all 254 finite codes, unit scales:
    down + combine is exact, gate/up within one bf16 ulp of silu(g) * u."""
    E, N, K, M = 2, 64, 128, 16
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    q8 = codes[torch.arange(E * N * K) % 254].view(E, N, K)
    q = q8.cuda().view(torch.float8_e4m3fn)
    want = q8.view(torch.float8_e4m3fn).float()  # CPU decode
    qg = torch.full((E, N, K), 0x3C, dtype=torch.uint8).cuda().view(
        torch.float8_e4m3fn)  # 0x3c = 1.5
    one = torch.ones(E, N, device="cuda")
    idx = torch.tensor([[m % E] for m in range(M)], dtype=torch.int32).cuda()
    wts = torch.ones(M, 1, device="cuda")
    ws = torch.empty(16 * 64, device="cuda")
    rows = torch.arange(M)
    for c in range(K // M):
        x = torch.zeros(M, K)
        x[rows, c * M + rows] = 1.0  # row m hot at k = 16 c + m
        x = x.bfloat16().cuda()
        exp = want[rows % E, :, c * M + rows]  # [M, N]
        down = C.moe_combine(
            C.moe_down_fp8(x.view(1, M, K), idx, wts, q, one, ws, 1), x)
        assert torch.equal(down.float().cpu(), exp.bfloat16().float())
        got = C.moe_gate_up_swiglu_fp8(x, idx, qg, one, q, one)[0].float().cpu()
        ref = torch.nn.functional.silu(torch.tensor(1.5)) * exp
        ulp = ref.abs().clamp_min(2.0 ** -126) * 2.0 ** -7
        assert ((got - ref).abs() <= ulp).all()


def test_model_fp8_experts(monkeypatch):
    monkeypatch.setenv("REALHF_AMD_GEN_WEIGHT_QUANT", "fp8_e4m3")
    monkeypatch.delenv(KILL, raising=False)
    m = _mixtral("cuda", torch.bfloat16,
                 flat=_mixtral("cpu", torch.bfloat16).flat_param.data)
    calls = collections.Counter()
    for name in ("moe_route_decode", "moe_gate_up_swiglu", "moe_down",
                 "moe_gate_up_swiglu_fp8", "moe_down_fp8"):
        def spy(*a, _n=name, _f=getattr(C, name)):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(C, name, spy)

    tok_eager, lg_eager = _generate(monkeypatch, m, graph=False)
    n = calls["moe_route_decode"]  # one per layer and decode step
    assert n > 0 and calls == {"moe_route_decode": n, "moe_down_fp8": n,
                               "moe_gate_up_swiglu_fp8": n}
    m._gen_session = None
    tok_graph, lg0 = _generate(monkeypatch, m, graph=True)
    sess = m._gen_session[1]
    assert sess.decoder.graph is not None and all(sess.fp8.expert_pairs)
    assert torch.equal(tok_graph, tok_eager)

    with torch.no_grad():  # an in-place update, then refresh() under the graph
        torch.manual_seed(3)
        for name, t in m._params.items():
            if ".experts." in name:
                t.add_(0.03 * torch.randn_like(t))
    tok1, lg1 = _generate(monkeypatch, m, graph=True, forced=tok_graph)
    assert m._gen_session[1] is sess
    m._gen_session = None
    _, lg_fresh = _generate(monkeypatch, m, graph=False, forced=tok_graph)
    assert (lg1[1:] - lg0[1:]).abs().max().item() > 1e-2
    torch.testing.assert_close(lg1, lg_fresh, atol=3e-2, rtol=3e-2)

    calls.clear()
    monkeypatch.setenv(KILL, "1")
    _generate(monkeypatch, m, graph=False)
    assert calls == {"moe_route_decode": n, "moe_gate_up_swiglu": n,
                     "moe_down": n}
    assert m._gen_session[1].fp8.expert_pairs == [(), ()]


def test_quantization_error_no_worse_than_fp32_reference(monkeypatch):
    """Mean |dlogp| of 8 teacher-forced tokens, fp8 against unquantised: the
    kernels against an fp32 CPU copy with and without the dequantised weights,
    e_kernel <= 2 e_ref + 1e-3.  MI355X: e_kernel 3.13e-2, e_ref 2.85e-2."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models import generation as genmod

    monkeypatch.delenv("REALHF_AMD_GEN_WEIGHT_QUANT", raising=False)
    m = _mixtral("cuda", torch.bfloat16,
                 flat=_mixtral("cpu", torch.bfloat16).flat_param.data)
    forced = genmod.generate(m, *_prompts(), GenerationHyperparameters(
        max_new_tokens=9, greedy=True, use_hip_graph=False)).gen_tokens
    m32 = _mixtral("cpu", torch.float32, flat=m.flat_param.data.float().cpu())
    gaps, ref = [], ops.moe_decode_ref

    def ref_spy(h, rw, *a, **kw):
        top = (h @ rw.t()).sort(-1, descending=True).values
        gaps.append((top[:, 1] - top[:, 2]).min().item())
        return ref(h, rw, *a, **kw)

    with torch.no_grad():
        fp8, fp8_32 = genmod.Fp8DecodeWeights(m, 3), genmod.Fp8DecodeWeights(m32, 3)
        fp8.refresh(), fp8_32.refresh()
        assert all(fp8.expert_pairs) and all(fp8_32.expert_pairs)
        lp_bf16 = _teacher_forced(m, forced)
        lp_fp8 = _teacher_forced(m, forced, fp8)
        lp_32 = _teacher_forced(m32, forced)
        monkeypatch.setattr(ops, "moe_decode_ref", ref_spy)
        lp_32_fp8 = _teacher_forced(m32, forced, fp8_32)
    assert len(gaps) == 16 and min(gaps) >= 1e-2
    e_kernel = (lp_fp8 - lp_bf16).abs().mean().item()
    e_ref = (lp_32_fp8 - lp_32).abs().mean().item()
    print(f"mean |dlogp| fp8 - unquantized: {e_kernel:.4e}, fp32 CPU {e_ref:.4e}")
    assert 0 < e_kernel <= 2 * e_ref + 1e-3
