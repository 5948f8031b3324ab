#!/usr/bin/env python3
"""MoE decode A/B, one process.  Run on an MI355X.

1. One MoE layer's decode MLP (router, experts, combine with the residual) on
   the moe_decode kernels against REALHF_AMD_NO_MOE_DECODE=1, the training
   route MoELayer.forward, at batch 1, 4 and 16 for a Mixtral-8x7B layer
   (H 4096, I 14336, E 8, k 2) and a Qwen3-MoE-like one (H 2048, I 768, E 128,
   k 8).  Each call takes the next of --inputs distinct token batches, so
   successive calls route to different experts and stream their weights from
   HBM, as successive layers of a model do.  Effective TB/s counts the bf16
   gate, up and down weights of the experts the batch actually chose.
2. generate() of a tiny mixtral: kernels under the captured graph, kernels
   eager, and the kill switch (eager: it cannot be captured).

--fp8 [--shape NAME] runs instead the same layers, M and rotating inputs with
e4m3 expert pairs (moe_gate_up_swiglu_fp8, moe_down_fp8) against the bf16
expert kernels, alternating in one run; TB/s then counts code bytes.

Every figure is min / median / max over --repeats timed windows; the arms of
a comparison alternate inside each repeat.  The training route syncs with
the host in every call, so all arms are timed by the wall clock."""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

import realhf_amd._C as C
from realhf_amd.api.model import GenerationHyperparameters, MoEConfig
from realhf_amd.models import generation as genmod
from realhf_amd.models.hf import get_family
from realhf_amd.models.moe import MoELayer
from realhf_amd.models.real_model import ReaLModel

KILL = "REALHF_AMD_NO_MOE_DECODE"
SHAPES = [  # (name, H, I, E, k)
    ("mixtral-8x7b", 4096, 14336, 8, 2),
    ("qwen3-moe-like", 2048, 768, 128, 8),
]


def window(fn, iters, warmup):
    """µs per call over one timed window that ends in a synchronise."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def stats(ts):
    return min(ts), statistics.median(ts), max(ts)


def make_layer(H, I, E, k):
    cfg = get_family("mixtral").make_test_config(
        n_layers=1, hidden_dim=H, n_heads=H // 128, n_kv_heads=H // 128,
        head_dim=128, vocab_size=256, intermediate_dim=I)
    cfg.moe = MoEConfig(num_experts=E, top_k=k)
    flat = torch.empty(E * H + 3 * E * H * I, dtype=torch.bfloat16, device="cuda")
    params, off = {}, 0

    def take(name, n, kk, scale):
        nonlocal off
        w = flat[off:off + n * kk].view(n, kk)
        w.copy_(torch.randn(n, kk, device="cuda") * scale)
        params[name] = w
        off += n * kk

    take("1.mlp.router.weight", E, H, 4 / math.sqrt(H))
    for e in range(E):
        take(f"1.mlp.experts.{e}.gate.weight", I, H, 1 / math.sqrt(H))
        take(f"1.mlp.experts.{e}.up.weight", I, H, 1 / math.sqrt(H))
        take(f"1.mlp.experts.{e}.down.weight", H, I, 1 / math.sqrt(I))
    return MoELayer(cfg, 1, params, tp_size=1).eval()


@torch.no_grad()
def bench_layer_fp8(a):
    """--fp8: the same layers, inputs and M with e4m3 expert pairs installed
    (moe_gate_up_swiglu_fp8, moe_down_fp8) against the bf16 kernels in the
    same run.  TB/s counts the code bytes of the experts in use."""
    from realhf_amd.ops import functional as ops

    print(f"one MoE layer's decode MLP, FP8 against bf16 expert kernels, "
          f"iters={a.iters} x repeats={a.repeats}, {a.inputs} rotating inputs; "
          "us per call (min / median / max)")
    print(f"{'shape':16} {'M':>3} {'fp8 kernels us':>26} {'bf16 kernels us':>26} "
          f"{'ratio':>6} {'experts':>8} {'TB/s':>6}")
    for name, H, I, E, k in SHAPES:
        if a.shape not in ("all", name):
            continue
        torch.manual_seed(0)
        layer = make_layer(H, I, E, k)
        pairs = tuple(ops.quantize_rows_e4m3(w) for w in layer.decode_stacks())
        for M in (1, 4, 16):
            hs = [torch.randn(M, H, device="cuda").bfloat16()
                  for _ in range(a.inputs)]
            res = torch.randn(M, H, device="cuda").bfloat16()
            n_active = statistics.mean(
                C.moe_route_decode(h, layer.router.weight, k, True)[0]
                .unique().numel() for h in hs)
            fn = lambda i: layer.decode(hs[i % a.inputs], residual=res)
            t_new, t_old = [], []
            for _ in range(a.repeats):
                layer.fp8 = pairs
                t_new.append(window(fn, a.iters, a.iters // 10))
                layer.fp8 = ()
                t_old.append(window(fn, a.iters, a.iters // 10))
            fmt = lambda s: f"{s[0]:8.1f}/{s[1]:8.1f}/{s[2]:8.1f}"
            new, old = stats(t_new), stats(t_old)
            tbs = n_active * 3 * H * I / (new[1] * 1e-6) / 1e12
            print(f"{name:16} {M:3d} {fmt(new)} {fmt(old)} "
                  f"{old[1] / new[1]:6.2f} {n_active:8.1f} {tbs:6.2f}")
        del layer, pairs
        torch.cuda.empty_cache()


@torch.no_grad()
def bench_layer(a):
    print(f"one MoE layer's decode MLP, iters={a.iters} x repeats={a.repeats}, "
          f"{a.inputs} rotating inputs; us per call (min / median / max)")
    print(f"{'shape':16} {'M':>3} {'kernels us':>26} {'training route us':>26} "
          f"{'ratio':>6} {'experts':>8} {'TB/s':>6}")
    for name, H, I, E, k in SHAPES:
        torch.manual_seed(0)
        layer = make_layer(H, I, E, k)
        for M in (1, 4, 16):
            hs = [torch.randn(M, H, device="cuda").bfloat16()
                  for _ in range(a.inputs)]
            res = torch.randn(M, H, device="cuda").bfloat16()
            n_active = statistics.mean(
                C.moe_route_decode(h, layer.router.weight, k, True)[0]
                .unique().numel() for h in hs)
            assert layer.decode_supported(torch.bfloat16, "cuda")
            fn = lambda i: layer.decode(hs[i % a.inputs], residual=res)
            t_new, t_old = [], []
            for _ in range(a.repeats):
                os.environ.pop(KILL, None)
                t_new.append(window(fn, a.iters, a.iters // 10))
                os.environ[KILL] = "1"
                t_old.append(window(fn, a.iters, a.iters // 10))
            os.environ.pop(KILL, None)
            fmt = lambda s: f"{s[0]:8.1f}/{s[1]:8.1f}/{s[2]:8.1f}"
            new, old = stats(t_new), stats(t_old)
            tbs = n_active * 3 * H * I * 2 / (new[1] * 1e-6) / 1e12
            print(f"{name:16} {M:3d} {fmt(new)} {fmt(old)} "
                  f"{old[1] / new[1]:6.2f} {n_active:8.1f} {tbs:6.2f}")
        del layer
        torch.cuda.empty_cache()


def bench_generate(a):
    cfg = get_family("mixtral").make_test_config(
        n_layers=2, hidden_dim=256, n_heads=4, n_kv_heads=4, head_dim=64,
        vocab_size=256, intermediate_dim=192)
    cfg.family = "mixtral"
    torch.manual_seed(0)
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    m.random_init(std=0.05)
    toks = torch.randint(0, 256, (26,), device="cuda")
    cu = torch.tensor([0, 12, 21, 26], dtype=torch.int32, device="cuda")
    arms = [("kernels, graph", None, True), ("kernels, eager", None, False),
            ("training route, eager", "1", False)]
    ts = {n: [] for n, _, _ in arms}
    for r in range(a.repeats + 1):  # the first round warms up (and captures)
        for n, kill, graph in arms:
            os.environ.pop(KILL, None)
            if kill:
                os.environ[KILL] = kill
            g = GenerationHyperparameters(max_new_tokens=a.new_tokens,
                                          greedy=True, use_hip_graph=graph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            genmod.generate(m, toks, cu, g)
            torch.cuda.synchronize()
            if r:
                ts[n].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop(KILL, None)
    print(f"\ntiny mixtral generate(), 3 prompts, {a.new_tokens} new tokens; "
          "ms (min / median / max)")
    for n, _, _ in arms:
        s = stats(ts[n])
        print(f"{n:24} {s[0]:8.2f}/{s[1]:8.2f}/{s[2]:8.2f}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200, help="calls per window")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--inputs", type=int, default=16)
    p.add_argument("--new-tokens", type=int, default=64)
    p.add_argument("--fp8", action="store_true",
                   help="FP8 expert kernels against the bf16 kernels, only")
    p.add_argument("--shape", default="all",
                   choices=["all"] + [s[0] for s in SHAPES],
                   help="with --fp8: one shape per process")
    a = p.parse_args()
    if a.fp8:
        bench_layer_fp8(a)
    else:
        bench_layer(a)
        bench_generate(a)
