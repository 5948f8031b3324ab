#!/usr/bin/env python3
"""Standalone A/B microbenchmark of qwen3's per-head QK RMSNorm on the HIP
path, at Qwen3-8B geometry (hidden 4096, 32 q heads, 8 kv heads, hd 128,
intermediate 12288), same process, alternating the paths call by call.

  train   qk_norm_rope forward + backward on views into a merged QKV buffer,
          fused kernel vs the kill-switch path (REALHF_AMD_NO_QK_NORM_OPS=1:
          torch norm + apply_rotary_ref under autograd), at 4 x 640 and
          16 x 2048 tokens, with the peak memory each call allocates.
  append  rope_qkv_decode_norm vs the un-normed rope_qkv_decode on the same
          split-K slabs at bs 16: what the norm adds to the launch.
  decode  one decode layer step at bs 16 inside a captured hipGraph, with and
          without the kill switch: the difference between a 5-layer and a
          1-layer model's graph replay, over 4.

Each path is timed as two interleaved series (a, b); the gap between the
medians of a and b of the SAME path is the run-to-run spread that a
difference between paths has to exceed to mean anything.

usage: bench_qk_norm.py [reps-per-series] [train|append|decode|all]
(needs a GPU; no fallback)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLAG = "REALHF_AMD_NO_QK_NORM_OPS"
H, I, NQ, NKV, HD = 4096, 12288, 32, 8, 128
TOKENS = (4 * 640, 16 * 2048)
EPS = 1e-6


def _event_ms(fn):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def _peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _ab(paths, reps):
    """paths: {name: fn}.  Two interleaved series per path."""
    series = {(p, s): [] for s in "ab" for p in paths}
    for _ in range(reps):
        for (p, s), v in series.items():
            v.append(_event_ms(paths[p]))
    out = {}
    for p in paths:
        a, b = series[(p, "a")], series[(p, "b")]
        ms = statistics.median(a + b)
        out[p] = {"ms": ms, "ms_a": statistics.median(a),
                  "ms_b": statistics.median(b), "min": min(a + b),
                  "max": max(a + b),
                  "spread": abs(statistics.median(a) - statistics.median(b)) / ms}
    return out


def _verdict(res, new, old):
    ratio = res[new]["ms"] / res[old]["ms"]
    spread = max(res[new]["spread"], res[old]["spread"])
    word = ("SLOWER beyond the spread" if ratio > 1 + spread else
            "faster beyond the spread" if ratio < 1 - spread else
            "within the spread")
    return ratio, spread, f"{new}/{old} = {ratio:.3f} (spread {100 * spread:.1f}%): {word}"


def _with_flag(kill, fn):
    def run():
        os.environ[FLAG] = "1" if kill else "0"
        return fn()
    return run


def bench_train(reps):
    from realhf_amd.ops import functional as F

    results = []
    print(f"{'tokens':>8} {'path':>7} {'ms a':>8} {'ms b':>8} {'min':>8} "
          f"{'max':>8} {'GB/s':>7} {'peak MiB':>9}")
    cos, sin = F.rotary_cache.get(HD, 4096, 1e6, "cuda")
    for n in TOKENS:
        torch.manual_seed(0)
        qkv = torch.randn(n, (NQ + 2 * NKV) * HD, device="cuda").to(
            torch.bfloat16).requires_grad_(True)
        q_w = (1 + 0.5 * torch.randn(HD, device="cuda")).to(
            torch.bfloat16).requires_grad_(True)
        k_w = (1 + 0.5 * torch.randn(HD, device="cuda")).to(
            torch.bfloat16).requires_grad_(True)
        gq = torch.randn(n, NQ, HD, device="cuda").to(torch.bfloat16)
        gk = torch.randn(n, NKV, HD, device="cuda").to(torch.bfloat16)
        pos = (torch.arange(n, device="cuda") % 2048)

        def step():
            q, k, _ = qkv.split([NQ * HD, NKV * HD, NKV * HD], dim=-1)
            qo, ko = F.qk_norm_rope(q.reshape(n, NQ, HD), k.reshape(n, NKV, HD),
                                    q_w, k_w, EPS, cos, sin, pos)
            return torch.autograd.grad([qo, ko], [qkv, q_w, k_w], [gq, gk])

        paths = {"torch": _with_flag(True, step), "hip": _with_flag(False, step)}
        for fn in paths.values():
            for _ in range(3):
                fn()
        res = _ab(paths, reps)
        # what the fused pair must move (bf16): fwd reads q, k, writes q', k';
        # bwd reads dq', dk', q, k, writes dq, dk
        nbytes = 12 * n * (NQ + NKV) * HD
        for p, r in res.items():
            r["peak_bytes"] = _peak_bytes(paths[p])
            r["GBps"] = nbytes / r["ms"] / 1e6
            print(f"{n:>8} {p:>7} {r['ms_a']:8.3f} {r['ms_b']:8.3f} "
                  f"{r['min']:8.3f} {r['max']:8.3f} {r['GBps']:7.0f} "
                  f"{r['peak_bytes'] / 2**20:9.1f}")
        v = _verdict(res, "hip", "torch")
        print(f"{'':>16} {v[2]}")
        results.append({"tokens": n, "bytes": nbytes, "paths": res,
                        "hip_over_torch": v[0]})
        del qkv, gq, gk
        torch.cuda.empty_cache()
    os.environ[FLAG] = "0"
    return results


def bench_append(reps, bs=16, maxlen=512, nks=8, calls=50):
    import realhf_amd._C as C
    from realhf_amd.ops import functional as F

    torch.manual_seed(0)
    cos, sin = F.rotary_cache.get(HD, maxlen, 1e6, "cuda")
    slabs = torch.randn(nks, bs, (NQ + 2 * NKV) * HD, device="cuda")
    q_w = (1 + 0.5 * torch.randn(HD, device="cuda")).to(torch.bfloat16)
    k_w = (1 + 0.5 * torch.randn(HD, device="cuda")).to(torch.bfloat16)
    kc = torch.zeros(bs, maxlen, NKV, HD, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    lens = torch.full((bs,), maxlen // 2, dtype=torch.int32, device="cuda")

    def many(fn):
        def run():
            for _ in range(calls):
                fn()
        return run

    paths = {
        "plain": many(lambda: C.rope_qkv_decode(
            slabs, None, kc, vc, lens, cos, sin, NQ, True)),
        "norm": many(lambda: C.rope_qkv_decode_norm(
            slabs, None, kc, vc, lens, cos, sin, NQ, True, q_w, k_w, EPS)),
    }
    for fn in paths.values():
        fn()
    res = _ab(paths, reps)
    print(f"{'append':>8} {'path':>7} {'us a':>8} {'us b':>8} {'min':>8} "
          f"{'max':>8}   (bs {bs}, {nks} slabs, per call incl. launch)")
    for p, r in res.items():
        print(f"{'':>8} {p:>7} " + " ".join(
            f"{r[k] / calls * 1e3:8.2f}" for k in ("ms_a", "ms_b", "min", "max")))
    v = _verdict(res, "norm", "plain")
    print(f"{'':>16} {v[2]}")
    return {"bs": bs, "nks": nks, "us_per_call": {
        p: r["ms"] / calls * 1e3 for p, r in res.items()},
        "paths": res, "norm_over_plain": v[0]}


def bench_decode(reps, bs=16, maxlen=512, replays=20):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.generation import DecodeGraph
    from realhf_amd.models.real_model import ReaLModel

    graphs = {}
    for L in (1, 5):
        cfg = hf_reg.get_family("qwen3").make_test_config(
            n_layers=L, hidden_dim=H, n_heads=NQ, n_kv_heads=NKV, head_dim=HD,
            vocab_size=256, intermediate_dim=I, max_position_embeddings=maxlen)
        cfg.family = "qwen3"
        torch.manual_seed(0)
        m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
        m.random_init()
        tokens = torch.randint(0, 256, (bs,), device="cuda")
        lens = torch.full((bs,), maxlen // 2, dtype=torch.int32, device="cuda")
        for kill in (False, True):
            os.environ[FLAG] = "1" if kill else "0"
            kv = [tuple(0.3 * torch.randn(bs, maxlen, NKV, HD, device="cuda")
                        .to(torch.bfloat16) for _ in range(2))
                  for _ in range(L)]
            d = DecodeGraph(m, kv, bs)
            with torch.no_grad():
                d.capture(tokens, lens)
            graphs[(L, kill)] = d
    os.environ[FLAG] = "0"  # the flag is baked into each captured graph

    def replay(d):
        def run():
            for _ in range(replays):
                d.graph.replay()
        return run

    paths = {f"{'torch' if kill else 'hip'}{L}": replay(d)
             for (L, kill), d in graphs.items()}
    for fn in paths.values():
        fn()
    res = _ab(paths, reps)
    row = {"bs": bs}
    print(f"{'decode layer':>14} {'path':>7} {'us a':>8} {'us b':>8} "
          f"{'min':>8} {'max':>8}   (bs {bs}, graph replay, per layer)")
    for p in ("torch", "hip"):
        per = {k: (res[p + "5"][k] - res[p + "1"][k]) / replays / 4 * 1e3
               for k in ("ms", "ms_a", "ms_b", "min", "max")}
        per["spread"] = abs(per["ms_a"] - per["ms_b"]) / per["ms"]
        row[p] = per
        print(f"{'qwen3-8b':>14} {p:>7} {per['ms_a']:8.1f} {per['ms_b']:8.1f} "
              f"{per['min']:8.1f} {per['max']:8.1f}")
    ratio = row["hip"]["ms"] / row["torch"]["ms"]
    spread = max(row["hip"]["spread"], row["torch"]["spread"])
    row["hip_over_torch"], row["spread"] = ratio, spread
    print(f"{'':>14} hip/torch = {ratio:.3f} (spread {100 * spread:.1f}%), "
          f"{row['torch']['ms'] - row['hip']['ms']:.1f} us per layer")
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm.py needs a GPU (no CPU fallback)")
    import realhf_amd._C  # noqa: F401 — the HIP extension must be built

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    what = sys.argv[2] if len(sys.argv) > 2 else "all"
    out = {}
    if what in ("train", "all"):
        out["train"] = bench_train(reps)
    if what in ("append", "all"):
        out["append"] = bench_append(reps)
    if what in ("decode", "all"):
        out["decode"] = bench_decode(reps)
    print(json.dumps({"bench_qk_norm": out}))


if __name__ == "__main__":
    main()
