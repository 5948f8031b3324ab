#!/usr/bin/env python3
"""Decode attention A/B: us and effective TB/s per context length.
REALHF_AMD_DEC_WAVES selects the wave-count variant (the kernel reads it
once per process, so A/B runs are one process per setting).

Without options: llama-7B geometry (32 heads x 128), the historical table.
--hd/--nq/--rep/--ctx pick another geometry (gemma-7B: --hd 256 --nq 16
--rep 1; gemma-2B: --hd 256 --nq 8 --rep 8) and print min/median/max over
--repeats timed windows; --ref also times the torch reference
(attn_decode_ref on the same bf16 tensors, the path a head dim without a
kernel takes)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
import realhf_amd._C as C


def bench(fn, iters=100, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    bs, nq, nkv, hd, maxlen = 16, 32, 32, 128, 704
    torch.manual_seed(0)
    q = (torch.randn(bs, nq, hd, device="cuda") * 0.3).to(torch.bfloat16)
    kc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 0.3).to(torch.bfloat16)
    vc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 0.3).to(torch.bfloat16)
    scale = hd ** -0.5
    print(f"waves={os.environ.get('REALHF_AMD_DEC_WAVES', '4(default)')}")
    print(f"{'ctx':>5} {'us':>8} {'TB/s':>6}")
    for ctx in (128, 256, 384, 512, 640):
        cs = torch.full((bs,), ctx, dtype=torch.int32, device="cuda")
        t = bench(lambda: C.attn_decode(q, kc, vc, cs, scale, 0))
        bytes_ = bs * nkv * ctx * hd * 2 * 2
        print(f"{ctx:5d} {t:8.1f} {bytes_ / t / 1e6:6.2f}")


def main_geometry(a):
    from realhf_amd.ops import functional as F

    bs, nq, hd = a.bs, a.nq, a.hd
    nkv = nq // a.rep
    maxlen = max(a.ctx) + 64
    torch.manual_seed(0)
    q = (torch.randn(bs, nq, hd, device="cuda") * 0.3).to(torch.bfloat16)
    kc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 0.3).to(torch.bfloat16)
    vc = (torch.randn(bs, maxlen, nkv, hd, device="cuda") * 0.3).to(torch.bfloat16)
    scale = hd ** -0.5
    print(f"waves={os.environ.get('REALHF_AMD_DEC_WAVES', 'default')} "
          f"bs={bs} nq={nq} nkv={nkv} hd={hd} repeats={a.repeats}")
    print(f"{'ctx':>6} {'path':>7} {'min us':>9} {'med us':>9} {'max us':>9} "
          f"{'TB/s(med)':>9}")
    for ctx in a.ctx:
        cs = torch.full((bs,), ctx, dtype=torch.int32, device="cuda")
        paths = [("hip", lambda: C.attn_decode(q, kc, vc, cs, scale, 0), a.iters)]
        if a.ref:
            paths.append(
                ("torch", lambda: F.attn_decode_ref(q, kc, vc, cs, scale),
                 max(3, a.iters // 20)))
        times = {name: [] for name, _, _ in paths}
        for _ in range(a.repeats):  # alternate the paths inside each repeat
            for name, fn, iters in paths:
                times[name].append(bench(fn, iters, warmup=max(2, iters // 10)))
        bytes_ = bs * nkv * ctx * hd * 2 * 2  # K and V rows read, bf16
        for name, _, _ in paths:
            ts = times[name]
            med = statistics.median(ts)
            print(f"{ctx:6d} {name:>7} {min(ts):9.1f} {med:9.1f} {max(ts):9.1f} "
                  f"{bytes_ / med / 1e6:9.2f}")


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--hd", type=int, default=None, help="head dim (64/128/256)")
    p.add_argument("--nq", type=int, default=16, help="query heads")
    p.add_argument("--rep", type=int, default=1, help="GQA ratio nq/nkv")
    p.add_argument("--bs", type=int, default=16)
    p.add_argument("--ctx", type=int, nargs="+", default=[640, 8192])
    p.add_argument("--iters", type=int, default=1000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--ref", action="store_true",
                   help="also time attn_decode_ref (torch) on the same inputs")
    a = p.parse_args()
    if a.hd is None:
        main()
    else:
        main_geometry(a)
