#!/usr/bin/env python3
"""Standalone A/B microbenchmark: fused vocab log-prob kernels
(REALHF_AMD_FUSED_LOGPROB=1) vs the torch path of
parallel.tp.packed_shifted_logprobs, forward + backward, same process,
alternating the two paths call by call.

Each path is timed as two interleaved series (a, b); the gap between the
medians of a and b of the SAME path is the run-to-run spread that a
fused-vs-torch difference has to exceed to mean anything.

Bytes are what the algorithm must move, computed from shapes: forward
reads the bf16 logits once (2nV), backward reads them and writes dlogits
(4nV).  GB/s = 6nV / time, against the ~6.3 TB/s achievable HBM figure.

usage: bench_logprob.py [reps-per-series]   (needs a GPU; no fallback)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_TBS = 6.3
SEQ = 640  # bench.py sequence length; every shape is n/640 packed sequences
SHAPES = [(2560, 32000), (10240, 32000), (2560, 152064)]
FLAG = "REALHF_AMD_FUSED_LOGPROB"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprob.py needs a GPU (no CPU fallback)")
    import realhf_amd._C  # noqa: F401 — the HIP extension must be built
    from realhf_amd.parallel.tp import packed_shifted_logprobs

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20

    def call(fused, x, cu, ids, go):
        os.environ[FLAG] = "1" if fused else "0"
        logp = packed_shifted_logprobs(x, cu, ids)
        return logp, torch.autograd.grad(logp, x, go)[0]

    def timed(fused, *args):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        call(fused, *args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop)

    def peak(fused, *args):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call(fused, *args)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    cases = []
    for n, V in SHAPES:
        torch.manual_seed(0)
        x = (torch.randn(n, V, device="cuda") * 4).to(torch.bfloat16)
        x.requires_grad_(True)
        ids = torch.randint(0, V, (n,), device="cuda")
        cu = torch.arange(0, n + 1, SEQ, dtype=torch.int32, device="cuda")
        go = torch.randn(n - n // SEQ, device="cuda")
        cases.append((n, V, (x, cu, ids, go)))
    for _, _, args in cases:  # warm up every shape on both paths
        for fused in (False, True):
            for _ in range(3):
                call(fused, *args)
    torch.cuda.synchronize()

    print(f"{'shape':>16} {'path':>6} {'ms a':>8} {'ms b':>8} {'min':>8} "
          f"{'max':>8} {'GB/s':>7} {'%6.3TB/s':>8} {'peak MiB':>9}")
    results = []
    for n, V, args in cases:
        series = {k: [] for k in ("torch_a", "fused_a", "torch_b", "fused_b")}
        for _ in range(reps):
            for k in series:
                series[k].append(timed(k.startswith("fused"), *args))
        nbytes = 6 * n * V
        row = {"n": n, "V": V, "bytes": nbytes}
        for path in ("torch", "fused"):
            a, b = series[path + "_a"], series[path + "_b"]
            ma, mb = statistics.median(a), statistics.median(b)
            ms = statistics.median(a + b)
            gbs = nbytes / ms / 1e6
            pk = peak(path == "fused", *args)
            row[path] = {
                "ms": ms, "ms_a": ma, "ms_b": mb, "min": min(a + b),
                "max": max(a + b), "spread": abs(ma - mb) / ms,
                "GBps": gbs, "peak_bytes": pk,
            }
            print(f"{f'{n}x{V}':>16} {path:>6} {ma:8.3f} {mb:8.3f} "
                  f"{min(a + b):8.3f} {max(a + b):8.3f} {gbs:7.0f} "
                  f"{100 * gbs / (ACHIEVABLE_TBS * 1e3):8.1f} "
                  f"{pk / 2**20:9.1f}")
        spread = max(row["torch"]["spread"], row["fused"]["spread"])
        ratio = row["fused"]["ms"] / row["torch"]["ms"]
        row["spread"], row["fused_over_torch"] = spread, ratio
        verdict = ("fused SLOWER than torch beyond the spread"
                   if ratio > 1 + spread else
                   "fused faster beyond the spread" if ratio < 1 - spread
                   else "within the spread")
        print(f"{'':>16} fused/torch = {ratio:.3f}, same-path spread "
              f"{100 * spread:.1f}% -> {verdict}")
        results.append(row)
    print(json.dumps({"bench_logprob": results}))


if __name__ == "__main__":
    main()
