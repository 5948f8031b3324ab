"""MoE decode on the HIP kernels (ops/csrc/moe_decode.hip): the router against
fp64, the routed expert path (gate/up + SwiGLU, down, slab combine) against
moe_decode_ref in fp64 from the same bf16 inputs, and a tiny mixtral through
generate() against the REALHF_AMD_NO_MOE_DECODE=1 route, eager and captured."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

KILL = "REALHF_AMD_NO_MOE_DECODE"


# ---------------------------------------------------------------------------
# router
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("norm_topk", [True, False])
@pytest.mark.parametrize("H", [256, 1088])
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 2), (128, 8)])
def test_router_matches_fp64(E, k, M, H, norm_topk):
    import realhf_amd._C as C

    torch.manual_seed(0)
    h = torch.randn(M, H).bfloat16()
    rw = (4 * torch.randn(E, H) / math.sqrt(H)).bfloat16()
    logits = h.double() @ rw.double().t()
    top = logits.sort(dim=-1, descending=True).values
    gap = (top[:, k - 1] - top[:, k]).min().item()
    assert gap >= 1e-3, gap  # the selection is well defined in fp32
    probs = torch.softmax(logits, -1)
    w_ref, i_ref = probs.topk(k, dim=-1)
    if norm_topk:
        w_ref = w_ref / w_ref.sum(-1, keepdim=True)
    ref = torch.zeros(M, E, dtype=torch.float64).scatter_(1, i_ref, w_ref)

    idx, wts = C.moe_route_decode(h.cuda(), rw.cuda(), k, norm_topk)
    assert idx.dtype == torch.int32 and wts.dtype == torch.float32
    got = torch.zeros(M, E, dtype=torch.float64).scatter_(
        1, idx.cpu().long(), wts.cpu().double())
    print("router gap", gap, "max |w diff|", (got - ref).abs().max().item())
    assert torch.equal(got > 0, ref > 0)
    assert (got - ref).abs().max().item() <= 1e-5


# ---------------------------------------------------------------------------
# expert path
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _weights(H, I, E):
    torch.manual_seed(0)
    mk = lambda n, k: (torch.randn(E, n, k, device="cuda") / math.sqrt(k)).bfloat16()
    return mk(I, H), mk(I, H), mk(H, I)


def _routing(kind, M, E, k):
    g = torch.Generator().manual_seed(1)
    if kind == "random":
        idx = torch.rand(M, E, generator=g).argsort(1)[:, :k]
    elif kind == "same":  # a full tile per active expert, the rest idle
        idx = (torch.arange(k) + 1).expand(M, k) % E
    else:  # "edge": expert 0 never, expert E-1 by the last token only
        idx = 1 + torch.rand(M, E - 2, generator=g).argsort(1)[:, :k]
        idx[M - 1, 0] = E - 1
    wts = torch.rand(M, k, generator=g) + 0.1
    wts = wts / wts.sum(-1, keepdim=True)
    return idx.int().contiguous().cuda(), wts.float().cuda()


@pytest.mark.parametrize("kind", ["random", "same", "edge"])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 2), (16, 8)])
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("H,I", [(256, 64), (256, 192), (1088, 1344)])
def test_expert_path_matches_fp64(H, I, M, E, k, kind):
    from realhf_amd.ops import functional as ops

    wg, wu, wd = (w.clone() for w in _weights(H, I, E))
    idx, wts = _routing(kind, M, E, k)
    idle = torch.ones(E, dtype=torch.bool, device="cuda")
    idle[idx.long().flatten()] = False
    for w in (wg, wu, wd):  # an idle expert must contribute nothing
        w[idle] = float("nan")
    torch.manual_seed(2)
    h = torch.randn(M, H, device="cuda").bfloat16()
    res = torch.randn(M, H, device="cuda").bfloat16()
    splitk = ops.moe_down_splitk(I)
    assert (splitk > 1) == (I > 1024)

    def run():  # every row consumed must have been written: NaN buffers
        act = torch.full((k, M, I), float("nan"), device="cuda",
                         dtype=torch.bfloat16)
        ws = torch.full((splitk * k * 16 * H,), float("nan"), device="cuda")
        return ops.moe_experts_decode(h, idx, wts, wg, wu, wd, residual=res,
                                      act=act, ws=ws)

    out = run()
    assert out.dtype == torch.bfloat16 and out.shape == (M, H)
    assert torch.isfinite(out).all()
    assert torch.equal(out, run())  # bitwise reproducible
    ref = ops.moe_decode_ref(
        h.double(), None, wg.double(), wu.double(), wd.double(), k, False,
        residual=res.double(), routing=(idx.long(), wts.double()))
    print("expert path max |diff|", (out.double() - ref).abs().max().item(),
          "max |ref|", ref.abs().max().item())
    torch.testing.assert_close(out.double(), ref, atol=3e-2, rtol=3e-2)


# ---------------------------------------------------------------------------
# model level: tiny mixtral, 2 layers, hidden 256, intermediate 192, 4 experts
# top-2, head dim 64
# ---------------------------------------------------------------------------
LENS = [12, 9, 5]
STEPS = 8
SEED = 0


def _mixtral(device, dtype, flat=None):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.moe import MoELayer
    from realhf_amd.models.real_model import ReaLModel

    cfg = hf_reg.get_family("mixtral").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=4, n_kv_heads=4, head_dim=64,
        vocab_size=256, intermediate_dim=192,
    )
    cfg.family = "mixtral"
    assert cfg.moe.num_experts == 4 and cfg.moe.top_k == 2
    m = ReaLModel(cfg, device=device, dtype=dtype)
    if flat is not None:
        m.flat_param.data.copy_(flat)
        return m
    torch.manual_seed(SEED)
    m.random_init(std=0.05)
    for layer in (x for x in m.modules() if isinstance(x, MoELayer)):
        w = layer.router.weight  # a view into the flat buffer
        w.data.copy_(4 * torch.randn(w.shape, device=device) / math.sqrt(w.shape[1]))
    return m


def _generate(monkeypatch, m, graph, forced=None, gaps=None):
    """generate() -> (tokens, [STEPS, bs, V] logits the sampler saw); forced:
    sample these tokens; gaps: collects every router call's smallest gap
    between the k-th and (k+1)-th logit."""
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models import generation as genmod
    from realhf_amd.models import moe as moe_mod

    seen = []
    real = genmod._sample_from_logits
    route = moe_mod.TopKRouter.forward

    def spy(logits, *a, **kw):
        tokens, logp, mask = real(logits, *a, **kw)
        if forced is not None:
            tokens = forced[:, len(seen)].to(tokens.device)
        seen.append(logits.clone())
        return tokens, logp, mask

    def route_spy(self, h):
        top = (h.float() @ self.weight.float().t()).sort(-1, descending=True).values
        k = self.moe.top_k
        gaps.append((top[:, k - 1] - top[:, k]).min().item())
        return route(self, h)

    dev = m.device
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 256, (sum(LENS),), generator=g).to(dev)
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32, device=dev)
    gconfig = GenerationHyperparameters(max_new_tokens=STEPS, greedy=True,
                                        use_hip_graph=graph)
    with monkeypatch.context() as mp:
        mp.setattr(genmod, "_sample_from_logits", spy)
        if gaps is not None:
            mp.setattr(moe_mod.TopKRouter, "forward", route_spy)
        out = genmod.generate(m, toks, cu, gconfig)
    return out.gen_tokens, torch.stack(seen)


def test_model_kernels_match_training_route(monkeypatch):
    monkeypatch.delenv(KILL, raising=False)
    # weights drawn on the CPU: the same model wherever the test runs
    m = _mixtral("cuda", torch.bfloat16,
                 flat=_mixtral("cpu", torch.bfloat16).flat_param.data)
    tok_eager, lg_eager = _generate(monkeypatch, m, graph=False)
    m._gen_session = None
    tok_graph, lg_graph = _generate(monkeypatch, m, graph=True)
    assert m._gen_session[1].decoder.graph is not None  # MoE under hipGraph
    assert torch.equal(tok_graph, tok_eager)

    # precondition: the routing is well separated along this token path
    m32 = _mixtral("cpu", torch.float32, flat=m.flat_param.data.float().cpu())
    gaps = []
    _generate(monkeypatch, m32, graph=False, forced=tok_eager.cpu(), gaps=gaps)
    print("smallest router top-k logit gap", min(gaps))
    assert min(gaps) >= 1e-2

    m._gen_session = None
    monkeypatch.setenv(KILL, "1")
    tok_ref, lg_ref = _generate(monkeypatch, m, graph=False)
    monkeypatch.delenv(KILL)
    assert torch.equal(tok_ref, tok_eager)
    print("moe kernels vs training route: max |diff|",
          (lg_eager - lg_ref).abs().max().item(), "max |logit|",
          lg_ref.abs().max().item())
    torch.testing.assert_close(lg_eager, lg_ref, atol=3e-2, rtol=3e-2)
