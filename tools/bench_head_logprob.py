#!/usr/bin/env python3
"""Standalone A/B microbenchmark: fused head log-probs
(ops.functional.head_logprobs, no logits) vs the logits route the model
takes today: _linear + final-logit cap + temperature +
packed_shifted_logprobs, once with REALHF_AMD_FUSED_LOGPROB off and once
with it on.  Forward only, under no_grad, same process, the three paths
alternating call by call.

Each path is timed as two interleaved series (a, b); the gap between the
medians of a and b of the SAME path is the run-to-run spread that a
difference between paths has to exceed to mean anything.

FLOPs are what the GEMM needs, 2 n H V, computed from shapes; TF/s is that
over the time of the whole call (GEMM + log-prob), not a kernel's share of
peak.  Peak MiB is the allocation above the pre-call level.

usage: bench_head_logprob.py [reps-per-series]   (needs a GPU; no fallback)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEQ = 640  # bench.py sequence length; every shape is n/640 packed sequences
TEMP = 0.7
# (n, H, V, final-logit cap)
SHAPES = [(2560, 4096, 32000, None), (2560, 4096, 152064, None),
          (10240, 4096, 152064, None), (2560, 2304, 256000, 30.0)]
FLAG = "REALHF_AMD_FUSED_LOGPROB"
PATHS = ("logits", "logits+lp", "fused")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_logprob.py needs a GPU (no CPU fallback)")
    import realhf_amd._C  # noqa: F401 — the HIP extension must be built
    from realhf_amd.models.layers import _linear
    from realhf_amd.ops import functional as F
    from realhf_amd.parallel.tp import (
        packed_next_token_labels,
        packed_shifted_logprobs,
    )

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10

    @torch.no_grad()
    def call(path, h, w, cu, ids, labels, leave, cap):
        if path == "fused":
            assert F.head_logprob_supported(h, w)
            return F.head_logprobs(h, w, labels, inv_temperature=1 / TEMP,
                                   softcap=cap)[leave]
        os.environ[FLAG] = "1" if path == "logits+lp" else "0"
        logits = _linear(h, w)
        if cap:
            logits = torch.tanh(logits / cap) * cap
        logits /= TEMP
        return packed_shifted_logprobs(logits, cu, ids)

    def timed(path, *args):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        call(path, *args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop)

    def peak(path, *args):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call(path, *args)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    print(f"{'n x H x V':>22} {'path':>10} {'ms a':>8} {'ms b':>8} {'min':>8} "
          f"{'max':>8} {'TF/s':>7} {'peak MiB':>9}")
    results = []
    for n, H, V, cap in SHAPES:  # one shape resident at a time
        torch.manual_seed(0)
        h = torch.randn(n, H, device="cuda").to(torch.bfloat16)
        w = (torch.randn(V, H, device="cuda") * 4 / H ** 0.5).to(torch.bfloat16)
        ids = torch.randint(0, V, (n,), device="cuda")
        cu = torch.arange(0, n + 1, SEQ, dtype=torch.int32, device="cuda")
        labels, leave = packed_next_token_labels(cu, ids)
        args = (h, w, cu, ids, labels, leave, cap)
        outs = {}
        for path in PATHS:  # warm up every path on this shape
            for _ in range(2):
                outs[path] = call(path, *args).float()
        series = {f"{p}_{s}": [] for s in "ab" for p in PATHS}
        for _ in range(reps):
            for k in series:
                series[k].append(timed(k[:-2], *args))
        flops = 2 * n * H * V
        row = {"n": n, "H": H, "V": V, "softcap": cap, "flops": flops,
               "max_abs_fused_minus_logits":
                   float((outs["fused"] - outs["logits"]).abs().max())}
        for path in PATHS:
            a, b = series[path + "_a"], series[path + "_b"]
            ma, mb = statistics.median(a), statistics.median(b)
            ms = statistics.median(a + b)
            pk = peak(path, *args)
            row[path] = {"ms": ms, "ms_a": ma, "ms_b": mb, "min": min(a + b),
                         "max": max(a + b), "spread": abs(ma - mb) / ms,
                         "TFps": flops / ms / 1e9, "peak_bytes": pk}
            print(f"{f'{n}x{H}x{V}':>22} {path:>10} {ma:8.3f} {mb:8.3f} "
                  f"{min(a + b):8.3f} {max(a + b):8.3f} "
                  f"{flops / ms / 1e9:7.0f} {pk / 2**20:9.1f}")
        spread = max(row[p]["spread"] for p in PATHS)
        for base in ("logits", "logits+lp"):
            ratio = row["fused"]["ms"] / row[base]["ms"]
            row[f"fused_over_{base}"] = ratio
            verdict = ("fused SLOWER beyond the spread" if ratio > 1 + spread
                       else "fused faster beyond the spread"
                       if ratio < 1 - spread else "within the spread")
            print(f"{'':>22} fused/{base} = {ratio:.3f}, same-path spread "
                  f"{100 * spread:.1f}% -> {verdict}")
        results.append(row)
        del h, w, outs
        torch.cuda.empty_cache()
    print(json.dumps({"bench_head_logprob": results}))


if __name__ == "__main__":
    main()
