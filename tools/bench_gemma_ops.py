#!/usr/bin/env python3
"""Standalone A/B microbenchmark: gemma's RMSNorm (1 + w) and GeGLU on the
HIP kernels vs the torch path (REALHF_AMD_NO_GEMMA_OPS=1), same process,
alternating the paths call by call, at gemma-2B and gemma-7B geometry.

  ops     norm forward+backward and GeGLU forward+backward at 2560 and
          16x2048 tokens, with the peak memory each call allocates.  The
          plain-RMS and SwiGLU kernels run next to them at the same shape:
          they move the same bytes, so they are what the new modes should
          cost.
  decode  one decode layer step at bs 16 inside a captured hipGraph: the
          difference between a 5-layer and a 1-layer model's graph replay,
          over 4.

Each path is timed as two interleaved series (a, b); the gap between the
medians of a and b of the SAME path is the run-to-run spread that a
difference between paths has to exceed to mean anything.

Bytes are what the algorithm must move, computed from shapes (bf16):
norm fwd reads x, writes out (4nH); bwd reads dy, x, writes dx (6nH);
GeGLU fwd reads gate_up, writes out (6nI); bwd reads dy, gate_up, writes
d(gate_up) (10nI).  GB/s is against the ~6.3 TB/s achievable HBM figure.

usage: bench_gemma_ops.py [reps-per-series] [ops|decode|all]
(needs a GPU; no fallback)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_TBS = 6.3
FLAG = "REALHF_AMD_NO_GEMMA_OPS"
#            name       H     I      heads kv
GEOMETRIES = [("gemma-2b", 2048, 16384, 8, 1),
              ("gemma-7b", 3072, 24576, 16, 16)]
TOKENS = (2560, 16 * 2048)
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


def bench_ops(reps):
    from realhf_amd.ops import functional as F

    def with_flag(kill, fn):
        def run():
            os.environ[FLAG] = "1" if kill else "0"
            return fn()
        return run

    print(f"{'op':>6} {'shape':>14} {'path':>7} {'ms a':>8} {'ms b':>8} "
          f"{'min':>8} {'max':>8} {'GB/s':>7} {'%6.3TB/s':>8} {'peak MiB':>9}")
    results = []
    for name, H, I, _, _ in GEOMETRIES:
        for n in TOKENS:
            torch.manual_seed(0)
            x = torch.randn(n, H, device="cuda").to(torch.bfloat16).requires_grad_(True)
            w = (0.1 * torch.randn(H, device="cuda")).to(torch.bfloat16).requires_grad_(True)
            gx = torch.randn(n, H, device="cuda").to(torch.bfloat16)
            gu = torch.randn(n, 2 * I, device="cuda").to(torch.bfloat16).requires_grad_(True)
            ga = torch.randn(n, I, device="cuda").to(torch.bfloat16)

            def norm(gemma):
                out = F.rms_norm(x, w, EPS, gemma_style=gemma)
                return torch.autograd.grad(out, (x, w), gx)

            def glu(fn):
                return torch.autograd.grad(fn(gu), gu, ga)

            ops = {
                "norm": (10 * n * H, {
                    "torch": with_flag(True, lambda: norm(True)),
                    "hip": with_flag(False, lambda: norm(True)),
                    "plain": with_flag(False, lambda: norm(False)),
                }),
                "geglu": (16 * n * I, {
                    "torch": with_flag(True, lambda: glu(F.geglu)),
                    "hip": with_flag(False, lambda: glu(F.geglu)),
                    "swiglu": with_flag(False, lambda: glu(F.swiglu)),
                }),
            }
            for op, (nbytes, paths) in ops.items():
                for fn in paths.values():  # warm up every path at this shape
                    for _ in range(3):
                        fn()
                res = _ab(paths, reps)
                twin = "plain" if op == "norm" else "swiglu"
                for p, r in res.items():
                    r["peak_bytes"] = _peak_bytes(paths[p])
                    r["GBps"] = nbytes / r["ms"] / 1e6
                    shape = f"{n}x{H if op == 'norm' else I}"
                    print(f"{op:>6} {shape:>14} {p:>7} {r['ms_a']:8.3f} {r['ms_b']:8.3f} "
                          f"{r['min']:8.3f} {r['max']:8.3f} {r['GBps']:7.0f} "
                          f"{100 * r['GBps'] / (ACHIEVABLE_TBS * 1e3):8.1f} "
                          f"{r['peak_bytes'] / 2**20:9.1f}")
                v_torch = _verdict(res, "hip", "torch")
                v_twin = _verdict(res, "hip", twin)
                print(f"{'':>21} {v_torch[2]}")
                print(f"{'':>21} {v_twin[2]}")
                results.append({"geometry": name, "op": op, "tokens": n,
                                "bytes": nbytes, "paths": res,
                                "hip_over_torch": v_torch[0],
                                "hip_over_twin": v_twin[0]})
            del x, w, gx, gu, ga
            torch.cuda.empty_cache()
    return results


def bench_decode(reps, bs=16, maxlen=512, replays=20):
    import realhf_amd.models.hf as hf_reg
    from realhf_amd.models.generation import DecodeGraph
    from realhf_amd.models.real_model import ReaLModel

    results = []
    print(f"{'decode layer':>14} {'path':>7} {'us a':>8} {'us b':>8} "
          f"{'min':>8} {'max':>8}   (bs {bs}, graph replay, per layer)")
    for name, H, I, nh, nkv in GEOMETRIES:
        graphs = {}
        for L in (1, 5):
            cfg = hf_reg.get_family("gemma").make_test_config(
                n_layers=L, hidden_dim=H, n_heads=nh, n_kv_heads=nkv,
                head_dim=256, vocab_size=256, intermediate_dim=I,
                max_position_embeddings=maxlen,
            )
            cfg.family = "gemma"
            torch.manual_seed(0)
            m = ReaLModel(cfg, device="cuda", dtype=torch.bfloat16)
            m.random_init()
            tokens = torch.randint(0, 256, (bs,), device="cuda")
            lens = torch.full((bs,), maxlen // 2, dtype=torch.int32, device="cuda")
            for kill in (False, True):
                os.environ[FLAG] = "1" if kill else "0"
                kv = [tuple(0.3 * torch.randn(bs, maxlen, nkv, 256, device="cuda")
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
        row = {"geometry": name, "bs": bs}
        for p in ("torch", "hip"):
            per = {k: (res[p + "5"][k] - res[p + "1"][k]) / replays / 4 * 1e3
                   for k in ("ms", "ms_a", "ms_b", "min", "max")}
            per["spread"] = abs(per["ms_a"] - per["ms_b"]) / per["ms"]
            row[p] = per
            print(f"{name:>14} {p:>7} {per['ms_a']:8.1f} {per['ms_b']:8.1f} "
                  f"{per['min']:8.1f} {per['max']:8.1f}")
        ratio = row["hip"]["ms"] / row["torch"]["ms"]
        spread = max(row["hip"]["spread"], row["torch"]["spread"])
        row["hip_over_torch"], row["spread"] = ratio, spread
        print(f"{'':>14} hip/torch = {ratio:.3f} (spread {100 * spread:.1f}%), "
              f"{row['torch']['ms'] - row['hip']['ms']:.1f} us per layer")
        results.append(row)
        del graphs, paths
        torch.cuda.empty_cache()
    return results


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemma_ops.py needs a GPU (no CPU fallback)")
    import realhf_amd._C  # noqa: F401 — the HIP extension must be built

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    what = sys.argv[2] if len(sys.argv) > 2 else "all"
    out = {}
    if what in ("ops", "all"):
        out["ops"] = bench_ops(reps)
    if what in ("decode", "all"):
        out["decode"] = bench_decode(reps)
    print(json.dumps({"bench_gemma_ops": out}))


if __name__ == "__main__":
    main()
