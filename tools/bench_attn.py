#!/usr/bin/env python3
"""Standalone A/B + profiling target for the flash-attention varlen
forward kernel.  `--hd N` instead compares forward and forward+backward of
the HIP kernels with the batched torch path at 16 heads x N."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import realhf_amd._C as C


def bench(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def run(shape_name, lens, nq, nkv, hd=128, iters=30):
    total = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32,
                      device="cuda")
    torch.manual_seed(0)
    q = (torch.randn(total, nq, hd, device="cuda") * 0.5).to(torch.bfloat16)
    k = (torch.randn(total, nkv, hd, device="cuda") * 0.5).to(torch.bfloat16)
    v = (torch.randn(total, nkv, hd, device="cuda") * 0.5).to(torch.bfloat16)
    scale = hd ** -0.5
    us = bench(lambda: C.attn_varlen_fwd(q, k, v, cu, max(lens), True, scale, 0),
               iters)
    flops = sum(2 * 2 * (l * l / 2) * nq * hd for l in lens)
    print(f"{shape_name:24} {us:9.1f} us  {flops / us / 1e6:7.1f} TF/s")


def compare(shape_name, lens, nq, nkv, hd, iters=20, repeats=5):
    """HIP kernels (forward; forward + MFMA backward through the autograd
    function) against the batched-padded torch path on the same bf16
    inputs, alternating inside each repeat: median [min..max] us, TF/s at
    the median, peak extra memory of one call."""
    from realhf_amd.ops import functional as F

    total = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32,
                      device="cuda")
    torch.manual_seed(0)
    q, k, v = (
        (torch.randn(total, n, hd, device="cuda") * 0.5).to(torch.bfloat16)
        .requires_grad_(True) for n in (nq, nkv, nkv))
    g = (torch.randn(total, nq, hd, device="cuda") * 0.5).to(torch.bfloat16)
    scale = hd ** -0.5
    ms = max(lens)

    def hip():
        return F._AttnVarlenFn.apply(q, k, v, cu, ms, True, scale, None)

    def tor():
        return F._attn_varlen_blocked_torch(q, k, v, cu, True, scale)

    def fwd(f):
        with torch.no_grad():
            f()

    def fwdbwd(f):
        torch.autograd.grad(f(), (q, k, v), g)

    fwd_flops = sum(2 * 2 * (l * l / 2) * nq * hd for l in lens)
    for mode, step, flops in (("fwd", fwd, fwd_flops),
                              ("fwd+bwd", fwdbwd, 3.5 * fwd_flops)):
        paths = (("hip", hip), ("torch", tor))
        # The torch path's backward hit an illegal memory access at
        # 16x2048 with 16 heads, where the padded fp32 score tensor
        # [bs, nh, Lmax, Lmax] is 4 GiB (docs/perf.md); its forward, and its
        # backward at 0.4 GiB, ran.  Not timed from 2 GiB up.
        score_bytes = len(lens) * nq * ms * ms * 4
        if mode == "fwd+bwd" and score_bytes >= 2 ** 31:
            paths = paths[:1]
            print(f"{shape_name:22} hd{hd} {mode:8} torch  not run: "
                  f"{score_bytes / 2 ** 30:.1f} GiB padded score tensor")
        times = {n: [] for n, _ in paths}
        peak = {}
        for _ in range(repeats):
            for n, f in paths:
                times[n].append(bench(lambda: step(f), iters))
        for n, f in paths:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(f)
            torch.cuda.synchronize()
            peak[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for n, _ in paths:
            ts = sorted(times[n])
            med = ts[len(ts) // 2]
            print(f"{shape_name:22} hd{hd} {mode:8} {n:6} {med:10.1f} us "
                  f"[{ts[0]:.1f}..{ts[-1]:.1f}]  {flops / med / 1e6:7.1f} TF/s  "
                  f"peak +{peak[n]:.0f} MiB")


if __name__ == "__main__":
    import argparse

    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("iters", type=int, nargs="?", default=None)
    p.add_argument("--hd", type=int, default=None,
                   help="head dim: compare the HIP kernels with the torch "
                        "path at 16 heads x hd (gemma-7B at 256)")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--shapes", nargs="+", default=["4x640", "16x640", "16x2048"],
                   help="with --hd: BSxLEN shapes to compare")
    a = p.parse_args()
    if a.hd is not None:
        it = a.iters or 20
        for shape in a.shapes:
            bs, ln = (int(x) for x in shape.split("x"))
            compare(f"{shape} h16", [ln] * bs, 16, 16, a.hd, it, a.repeats)
        sys.exit(0)
    iters = a.iters if a.iters is not None else 30
    run("bench-mb 4x640 h32", [640] * 4, 32, 32, iters=iters)
    run("bench-full 16x640 h32", [640] * 16, 32, 32, iters=iters)
    run("long 16x2048 h32gqa8", [2048] * 16, 32, 8, iters=iters)
    # long-context tier (device-built block lists; grad-ckpt training
    # shapes for the CP/packing long-context story)
    run("16k 2x16384 h32gqa8", [16384] * 2, 32, 8, iters=max(3, iters // 6))
    run("32k 1x32768 h32gqa8", [32768], 32, 8, iters=max(3, iters // 10))
