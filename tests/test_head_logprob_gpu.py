"""Fused head GEMM + log-sum-exp kernel (ops/csrc/head_logprob.hip) against
fp64 torch on the same bf16 values, at the smallest shapes at which each
mechanism can break.  Bound: assert_logp_close (atol = rtol = 1e-4); every
case first holds the fp32 torch chain to it, so a failure is the kernel's.
All tests require an MI355X."""
import copy
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

import realhf_amd._C as C  # noqa: E402 — must exist on a GPU box
from realhf_amd.ops import functional as F  # noqa: E402
from tests.test_fused_logprob import assert_logp_close, hand_combine  # noqa: E402

BF16 = torch.bfloat16
FLAG = "REALHF_AMD_FUSED_HEAD_LOGPROB"
# (n, H, V, nsplit)
CASES = [
    (1, 64, 8, 1),          # one partial tile in every dimension
    (17, 96, 136, 1),       # K tail (64 + 32), vocab tail past one tile
    (130, 64, 128, 1),      # second row block with 2 live rows, exact tile
    (129, 512, 2056, 1),    # many K steps, many tiles with running rescale
    (129, 512, 2056, 3),    # uneven splits (6, 6, 5 tiles)
    (5, 128, 50257, 0),     # odd vocab, heuristic splits
]
WARPS = [{}, {"softcap": 2.0}, {"inv_temperature": 1 / 0.7}]
_cache = {}


def case(n, H, V):
    """(h, w, labels) on the GPU: logits ~ N(0, 4^2); the labels start with
    0, V - 1, an ignored row and both sides of the tile boundary, as far as
    n and V allow."""
    if (n, H, V) not in _cache:
        g = torch.Generator().manual_seed(n * 1000 + V)
        h = torch.randn(n, H, generator=g).to(BF16).cuda()
        w = (torch.randn(V, H, generator=g) * 4 / H ** 0.5).to(BF16).cuda()
        labels = torch.randint(0, V, (n,), generator=g)
        special = [0, V - 1, -100] + [c for c in (127, 128) if c < V]
        labels[:len(special)] = torch.tensor(special)[:n]
        _cache[(n, H, V)] = (h, w, labels.cuda())
    return _cache[(n, H, V)]


def reference(h, w, labels, dtype, **kw):
    logp, _ = F.combine_vocab_stats(
        *F.head_logprobs_ref(h.to(dtype), w.to(dtype), labels, **kw))
    return logp.masked_fill(labels == -100, 0.0).float()


def kernel(h, w, labels, nsplit=0, vocab_start=0, softcap=None,
           inv_temperature=1.0):
    return C.head_logprob_fwd(h, w, labels, vocab_start, -100, inv_temperature,
                              softcap or 0.0, nsplit)


@pytest.mark.parametrize("warp", WARPS, ids=["plain", "cap", "temp"])
@pytest.mark.parametrize("n,H,V,nsplit", CASES)
def test_forward(n, H, V, nsplit, warp):
    h, w, labels = case(n, H, V)
    want = reference(h, w, labels, torch.float64, **warp)
    assert_logp_close(reference(h, w, labels, torch.float32, **warp), want)
    if warp:  # an ignored argument cannot pass
        with pytest.raises(AssertionError):
            assert_logp_close(reference(h, w, labels, torch.float64), want)
    stats = kernel(h, w, labels, nsplit, **warp)
    assert all(s.dtype == torch.float32 and s.shape == (n,) for s in stats)
    ign = labels == -100
    assert all(torch.equal(s[ign], torch.full_like(s[ign], v))
               for s, v in zip(stats, (0.0, 0.0, 1.0)))
    got = F.combine_vocab_stats(*stats)[0].masked_fill(ign, 0.0)
    print("max |kernel - fp64|", float((got - want).abs().max()))
    assert_logp_close(got, want)
    if nsplit == 0:  # the public op is the same numbers
        with torch.no_grad():
            assert torch.equal(F.head_logprobs(h, w, labels, **warp), got)


def test_vocab_slices():
    h, w, labels = case(17, 96, 136)
    kw = {"softcap": 2.0, "inv_temperature": 1 / 0.7}
    lo, hi = w[:72], w[72:]  # hi starts 16-byte aligned: 72 * 96 * 2 bytes
    parts = [kernel(h, lo, labels, vocab_start=0, **kw),
             kernel(h, hi, labels, vocab_start=72, **kw)]
    assert parts[1][0][0] == 0 and parts[0][0][1] == 0  # label outside the slice
    keep = labels != -100
    logp, _ = hand_combine(parts)
    whole, _ = F.combine_vocab_stats(*kernel(h, w, labels, **kw))
    assert_logp_close(logp[keep], whole[keep])
    assert_logp_close(logp[keep],
                      reference(h, w, labels, torch.float64, **kw)[keep])


def test_run_to_run_and_strided_w():
    h, w, labels = case(129, 512, 2056)
    a = kernel(h, w, labels, 3, softcap=2.0)
    b = kernel(h, w, labels, 3, softcap=2.0)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    big = torch.zeros(2056, 1024, dtype=BF16, device="cuda")
    big[:, 512:] = float("nan")  # never read
    big[:, :512] = w
    view = big[:, :512]
    assert view.stride(0) == 1024 and not view.is_contiguous()
    c = kernel(h, view, labels, 3, softcap=2.0)
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def _peak(fn):
    """Peak allocation above the pre-call level during fn()."""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_memory():
    """A condition of the design: the fused route allocates the outputs and
    the [nsplit <= 64, 3, n] fp32 workspace, never n * V of anything."""
    n, H, V = 256, 256, 32000
    h, w, labels = case(n, H, V)
    with torch.no_grad():
        fused, _ = _peak(lambda: F.head_logprobs(h, w, labels))
    with torch.enable_grad():  # the kernel's gate is closed: logits route
        plain, _ = _peak(lambda: F.head_logprobs(h, w, labels))
    print("peaks", fused, plain, "n*V*2 =", n * V * 2)
    assert fused < n * V * 2 / 10
    assert plain > n * V * 2


@pytest.mark.parametrize("family,cfg_kw", [
    ("gemma2", {"final_logit_softcap": 3.0}), ("llama", {})])
def test_model_inference(family, cfg_kw, monkeypatch):
    """PPO inference of a tiny bf16 model, packed 33 + 64 tokens, temperature
    0.7, flag off and on, each against an fp32 CPU copy of the model."""
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.api.config import ModelName
    from realhf_amd.api.data import SequenceSample
    from realhf_amd.api.model import Model
    from realhf_amd.models.real_model import ReaLModel
    from tests.test_head_logprob import _iface
    from tests.test_interfaces import init_inf

    V = 32000
    cfg = hf_reg.get_family(family).make_test_config(
        n_layers=2, hidden_dim=256, n_heads=2, n_kv_heads=1, head_dim=128,
        vocab_size=V, intermediate_dim=512, **cfg_kw)
    cfg.family = family
    torch.manual_seed(7)
    m = ReaLModel(cfg, device="cuda", dtype=BF16)
    m.random_init()
    cfg32 = copy.deepcopy(cfg)
    cfg32.dtype = "float32"
    m32 = ReaLModel(cfg32, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        m32.flat_param.copy_(m.flat_param.float().cpu())
    toks = torch.from_numpy(np.random.RandomState(3).randint(0, V, size=97))
    iface = _iface("ppo_actor", 0.7)

    def run(module, device, dtype):
        model = init_inf(Model(name=ModelName("ref", 0), module=module,
                               tokenizer=None, device=torch.device(device),
                               dtype=dtype))
        batch = SequenceSample(
            keys=("packed_input_ids",), ids=["a", "b"],
            seqlens={"packed_input_ids": [[33], [64]]},
            data={"packed_input_ids": toks.long().to(device)})
        peak, out = _peak(lambda: iface.inference(model, batch)
                          .data["packed_ref_logprobs"].float().cpu())
        assert out.shape == (95,) and torch.isfinite(out).all()
        return peak, out

    monkeypatch.delenv(FLAG, raising=False)
    _, want = run(m32, "cpu", torch.float32)
    peak_off, off = run(m, "cuda", BF16)
    monkeypatch.setenv(FLAG, "1")
    peak_on, on = run(m, "cuda", BF16)
    err_off = float((off - want).abs().max())
    err_on = float((on - want).abs().max())
    print(family, "err off/on", err_off, err_on, "peak off/on", peak_off, peak_on)
    assert err_on <= 2 * err_off + 1e-3
    assert peak_on < 97 * V * 2 <= peak_off  # no [total, vocab] tensor
