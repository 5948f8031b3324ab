#!/usr/bin/env python3
"""Standalone A/B microbenchmark: the sample_logits kernel against the torch
sampler of models.generation (_sample_from_logits), one decode step's
sampling on [bs, V] bf16 logits, same process, alternating the two paths
call by call, device events after warm-up.

The torch path is timed as generate() runs it, the fp32 copy of the logits
included; the kernel reads the bf16 rows and one torch.rand(bs).  Where
sample_logits_unsupported names a reason the "hip" rows are sample_logits_ref,
as sampler="hip" runs it, and the row says so.  Each path
is timed as two interleaved series (a, b); the gap between the medians of a
and b of the SAME path is the run-to-run spread that a difference has to
exceed to mean anything.  Times are GPU time between events around eagerly
issued launches, so launch gaps that the GPU waits through are included.

usage: bench_sampler.py [reps-per-series]   (needs a GPU; no fallback)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BS = 16
SHAPES = [32000, 128256]
FILTERS = [(1000, 0.9), (200, 1.0), (0, 1.0),  # top_k 0 = off
           (0, 0.9), (0, 0.99), (4000, 0.9)]  # the kernel's search form


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler.py needs a GPU (no CPU fallback)")
    import realhf_amd._C  # noqa: F401 — the HIP extension must be built
    from realhf_amd.api.model import GenerationHyperparameters
    from realhf_amd.models.generation import _sample_from_logits
    from realhf_amd.ops import functional as F

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    gen = torch.Generator("cuda").manual_seed(0)

    def call(hip, x, g):
        if hip:
            u = torch.rand(BS, generator=gen, device="cuda")
            return F.sample_logits(x, u, g.temperature, g.top_k, g.top_p)
        return _sample_from_logits(x.float(), g, gen)

    def timed(hip, x, g):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        call(hip, x, g)
        stop.record()
        torch.cuda.synchronize()
        return 1e3 * start.elapsed_time(stop)

    cases = []
    for V in SHAPES:
        torch.manual_seed(0)
        x = (torch.randn(BS, V, device="cuda") * 4).to(torch.bfloat16)
        for k, p in FILTERS:
            g = GenerationHyperparameters(top_k=k, top_p=p, temperature=1.0)
            cases.append((V, k, p, x, g))
    for *_, x, g in cases:  # warm up every shape on both paths
        for hip in (False, True):
            for _ in range(5):
                call(hip, x, g)
    torch.cuda.synchronize()

    print(f"{'V':>7} {'top_k':>6} {'top_p':>5} {'path':>6} {'us a':>8} "
          f"{'us b':>8} {'min':>8} {'max':>8}")
    results = []
    for V, k, p, x, g in cases:
        series = {n: [] for n in ("torch_a", "hip_a", "torch_b", "hip_b")}
        for _ in range(reps):
            for n in series:
                series[n].append(timed(n.startswith("hip"), x, g))
        # a request the gate names runs sample_logits_ref under sampler="hip"
        why = F.sample_logits_unsupported(x, k, p, False)
        row = {"bs": BS, "V": V, "top_k": k, "top_p": p, "hip_is_reference": why}
        if why is not None:
            print(f"{'':>20} hip = sample_logits_ref ({why})")
        for path in ("torch", "hip"):
            a, b = series[path + "_a"], series[path + "_b"]
            ma, mb = statistics.median(a), statistics.median(b)
            us = statistics.median(a + b)
            row[path] = {"us": us, "us_a": ma, "us_b": mb, "min": min(a + b),
                         "max": max(a + b), "spread": abs(ma - mb) / us}
            print(f"{V:>7} {k:>6} {p:>5} {path:>6} {ma:8.1f} {mb:8.1f} "
                  f"{min(a + b):8.1f} {max(a + b):8.1f}")
        spread = max(row["torch"]["spread"], row["hip"]["spread"])
        ratio = row["hip"]["us"] / row["torch"]["us"]
        row["spread"], row["hip_over_torch"] = spread, ratio
        verdict = ("hip SLOWER than torch beyond the spread"
                   if ratio > 1 + spread else
                   "hip faster beyond the spread" if ratio < 1 - spread
                   else "within the spread")
        print(f"{'':>20} hip/torch = {ratio:.3f}, same-path spread "
              f"{100 * spread:.1f}% -> {verdict}")
        results.append(row)
    print(json.dumps({"bench_sampler": results}))


if __name__ == "__main__":
    main()
