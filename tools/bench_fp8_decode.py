#!/usr/bin/env python3
"""FP8 weight-only decode A/B, one process.  Run on an MI355X.

1. The four llama-7B decode projections at M = 16: bf16 skinny GEMM against
   the fp8-weight one, slab (`_nc`) and combined entry points, in µs and
   effective weight bytes/s (N*K*2 for bf16, N*K + 4*N for fp8; x and the
   output are not counted).  Each shape rotates through enough distinct
   weight copies (--rotate-gb in total) that no launch finds its weights in
   the 256 MB last-level cache: in a real decode step 13 GB of weights
   stream through between two uses of the same matrix.
2. One decode step of an --layers-layer llama-7B-shaped model under the
   captured graph, bf16 weights against fp8, alternating.
3. The refresh: re-quantizing every decode projection of that model in place.

Every figure is min / median / max over --repeats timed windows; the two
arms of a comparison alternate inside each repeat."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

import realhf_amd._C as C
from realhf_amd.ops import functional as F

SHAPES = [  # (name, N, K): llama-7B, tp = 1
    ("qkv", 12288, 4096),
    ("o", 4096, 4096),
    ("gateup", 22016, 4096),
    ("down", 4096, 11008),
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


def bench_shapes(a):
    M = 16
    ws = torch.empty(2 * 16 * 16 * 22016, dtype=torch.float32, device="cuda")
    print(f"per-shape kernels, M={M}, iters={a.iters} x repeats={a.repeats}, "
          f"weights rotated over {a.rotate_gb} GB per arm")
    print(f"{'shape':7} {'N':>6} {'K':>6} {'sk':>3} {'entry':>9} "
          f"{'bf16 us min/med/max':>24} {'fp8 us min/med/max':>24} "
          f"{'bf16 TB/s':>9} {'fp8 TB/s':>9} {'bf16/fp8':>8}")
    for name, N, K in SHAPES:
        sk = F.skinny_splitk(K)  # what the model path chooses
        # the same number of copies in both arms; the fp8 arm alone spans
        # --rotate-gb, the bf16 arm twice that
        n = max(2, int(a.rotate_gb * 1e9 / (N * K)) + 1)
        torch.manual_seed(0)
        x = (torch.randn(M, K, device="cuda") * 0.3).to(torch.bfloat16)
        res = (torch.randn(M, N, device="cuda") * 0.3).to(torch.bfloat16)
        w = [(torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
             for _ in range(n)]
        p = [C.quantize_rows_e4m3(t) for t in w]
        arms = {
            "nc": (lambda i: C.skinny_gemm_nc(x, w[i % n], ws, sk),
                   lambda i: C.skinny_gemm_fp8_nc(x, *p[i % n], ws, sk)),
            "combined": (lambda i: C.skinny_gemm(x, w[i % n], ws, sk, res),
                         lambda i: C.skinny_gemm_fp8(x, *p[i % n], ws, sk, res)),
        }
        for entry, (f16, f8) in arms.items():
            t16, t8 = [], []
            for _ in range(a.repeats):
                t16.append(window(f16, a.iters, a.iters // 10))
                t8.append(window(f8, a.iters, a.iters // 10))
            s16, s8 = stats(t16), stats(t8)
            b16, b8 = N * K * 2, N * K + 4 * N
            print(f"{name:7} {N:6d} {K:6d} {sk:3d} {entry:>9} "
                  f"{s16[0]:8.1f}{s16[1]:8.1f}{s16[2]:8.1f} "
                  f"{s8[0]:8.1f}{s8[1]:8.1f}{s8[2]:8.1f} "
                  f"{b16 / s16[1] / 1e6:9.2f} {b8 / s8[1] / 1e6:9.2f} "
                  f"{s16[1] / s8[1]:8.2f}")
        del w, p
        torch.cuda.empty_cache()


def bench_model(a):
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models.generation import generate
    from realhf_amd.models.hf.llama import llama7b_config
    from realhf_amd.models.real_model import ReaLModel

    cfg = llama7b_config()
    cfg.n_layers = a.layers
    m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
    torch.manual_seed(0)
    m.random_init()
    bs, plen = 16, 128
    toks = torch.randint(0, cfg.vocab_size, (bs * plen,), device="cuda")
    cu = torch.arange(0, bs * plen + 1, plen, dtype=torch.int32, device="cuda")
    sessions = {}
    for quant in ("none", "fp8_e4m3"):
        g = GenerationHyperparameters(max_new_tokens=a.ctx_new, greedy=True,
                                      use_hip_graph=True, weight_quant=quant)
        generate(m, toks, cu, g)
        sessions[quant] = m._gen_session[1]  # keeps its graph and buffers
        assert sessions[quant].decoder.graph is not None, "no captured graph"
    torch.cuda.synchronize()
    fp8 = sessions["fp8_e4m3"].fp8
    print(f"\n{a.layers}-layer llama-7B-shaped model, bs={bs}, context "
          f"{plen + a.ctx_new}: fp8 decode weights {fp8.nbytes() / 1e9:.3f} GB "
          f"on top of {m.flat_param.numel() * 2 / 1e9:.3f} GB of bf16 parameters")

    t = {q: [] for q in sessions}
    for _ in range(a.repeats):
        for q, s in sessions.items():
            t[q].append(window(lambda i: s.decoder.graph.replay(),
                               a.step_iters, a.step_iters // 10))
    print(f"{'decode step (graph replay)':28} {'min us':>10} {'med us':>10} {'max us':>10}")
    for q in sessions:
        lo, med, hi = stats(t[q])
        print(f"{'weight_quant=' + q:28} {lo:10.1f} {med:10.1f} {hi:10.1f}")
    print(f"bf16 / fp8 (medians): "
          f"{statistics.median(t['none']) / statistics.median(t['fp8_e4m3']):.3f}")

    tr = [window(lambda i: fp8.refresh(), 3, 1) for _ in range(a.repeats)]
    lo, med, hi = stats(tr)
    nbytes = sum(q.numel() * 3 + 4 * s.numel()
                 for d in fp8.pairs for q, s in d.values())
    print(f"refresh of all {a.layers} layers: min/med/max "
          f"{lo / 1e3:.2f} / {med / 1e3:.2f} / {hi / 1e3:.2f} ms "
          f"({nbytes / 1e9:.2f} GB read once + written, "
          f"{nbytes / med / 1e6:.2f} TB/s; the second read of a row is an L2 hit)")


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawTextHelpFormatter)
    p.add_argument("--iters", type=int, default=2000, help="launches per window")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--rotate-gb", type=float, default=1.0)
    p.add_argument("--layers", type=int, default=32)
    p.add_argument("--ctx-new", type=int, default=384,
                   help="generated tokens before the step is timed")
    p.add_argument("--step-iters", type=int, default=100)
    p.add_argument("--skip-shapes", action="store_true")
    p.add_argument("--skip-model", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if not a.skip_shapes:
        bench_shapes(a)
    if not a.skip_model:
        bench_model(a)
