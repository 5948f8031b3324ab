#!/usr/bin/env python3
"""FP8 KV cache A/B, one process.  Run on an MI355X.

1. Decode attention: bf16 `attn_decode` against `attn_decode_fp8` on the same
   shapes, in µs and TB/s of attended K and V bytes (2*hd per key and cache
   for bf16, hd + 4 for fp8; q, the output and the split workspace are not
   counted).  Every sequence is full (cache_seqlens = ctx).  Each shape
   rotates through enough distinct caches (--rotate-gb per arm at least) that
   no launch finds its keys in the 256 MB last-level cache.
   REALHF_AMD_DEC_WAVES is read once per process: run one process per
   setting (--only-hd 256 limits the table to the gemma shapes).
2. The quantizing decode append against bf16 `rope_qkv_decode` and the
   quantizing prefill store against the bucketize + two index_put it
   replaces, at the flagship bench shape.
3. One decode step of an --layers-layer llama-7B-shaped model under the
   captured graph: bf16 / fp8 KV / fp8 KV + fp8 weights, alternating.

Every figure is min / median / max over --repeats timed windows; the arms of
a comparison alternate inside each repeat."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

import realhf_amd._C as C
from realhf_amd.ops import functional as F

ATTN_SHAPES = [  # (nq, nkv, hd, bs, ctx)
    (32, 32, 128, 16, 640),  # the flagship bench shape
    (32, 8, 128, 16, 2048),
    (32, 8, 128, 16, 8192),
    (32, 8, 128, 64, 2048),
    (32, 8, 128, 64, 8192),
    (16, 16, 256, 16, 640),
    (16, 16, 256, 16, 8192),
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


def fmt(s):
    return f"{s[0]:9.1f}{s[1]:9.1f}{s[2]:9.1f}"


def random_fp8_cache(bs, maxlen, nkv, hd):
    """Finite random codes (both signs) and scales around 2^-7."""
    codes = torch.randint(0, 0x7F, (bs, maxlen, nkv, hd), dtype=torch.uint8,
                          device="cuda")
    codes |= torch.randint(0, 2, codes.shape, dtype=torch.uint8,
                           device="cuda") << 7
    scale = torch.rand(bs, nkv, maxlen, device="cuda") * 2.0 ** -7 + 2.0 ** -8
    return F.Fp8KVCache(codes.view(torch.float8_e4m3fn), scale)


def bench_attention(a):
    print(f"decode attention, REALHF_AMD_DEC_WAVES="
          f"{os.environ.get('REALHF_AMD_DEC_WAVES', '(default 4)')}, "
          f"repeats={a.repeats}, caches rotated over >= {a.rotate_gb} GB per arm")
    print(f"{'nq/nkv':>7} {'hd':>4} {'bs':>3} {'ctx':>5} {'n':>3} "
          f"{'bf16 us min/med/max':>27} {'fp8 us min/med/max':>27} "
          f"{'bf16 TB/s':>9} {'fp8 TB/s':>9} {'bf16/fp8':>8}")
    for nq, nkv, hd, bs, ctx in ATTN_SHAPES:
        if a.only_hd and hd != a.only_hd:
            continue
        keys = bs * ctx * nkv
        b16, b8 = keys * 2 * hd * 2, keys * 2 * (hd + 4)
        n = max(2, int(a.rotate_gb * 1e9 / b8) + 1)
        torch.manual_seed(0)
        q = torch.randn(bs, nq, hd, device="cuda").to(torch.bfloat16)
        lens = torch.full((bs,), ctx, dtype=torch.int32, device="cuda")
        dense = [tuple((torch.randn(bs, ctx, nkv, hd, device="cuda") * 0.5)
                       .to(torch.bfloat16) for _ in range(2)) for _ in range(n)]
        quant = [tuple(random_fp8_cache(bs, ctx, nkv, hd) for _ in range(2))
                 for _ in range(n)]
        scale = hd ** -0.5

        def f16(i):
            k, v = dense[i % n]
            return C.attn_decode(q, k, v, lens, scale, 0)

        def f8(i):
            k, v = quant[i % n]
            return C.attn_decode_fp8(q, k.codes, k.scale, v.codes, v.scale,
                                     lens, scale, 0)

        # windows of about 0.2 s at 2 TB/s plus a launch floor
        iters = int(max(20, min(2000, 0.2 / (b16 / 2e12 + 2e-5))))
        t16, t8 = [], []
        for _ in range(a.repeats):
            t16.append(window(f16, iters, max(2, iters // 10)))
            t8.append(window(f8, iters, max(2, iters // 10)))
        s16, s8 = stats(t16), stats(t8)
        print(f"{nq:>4}/{nkv:<2} {hd:4d} {bs:3d} {ctx:5d} {n:3d} "
              f"{fmt(s16)} {fmt(s8)} {b16 / s16[1] / 1e6:9.2f} "
              f"{b8 / s8[1] / 1e6:9.2f} {s16[1] / s8[1]:8.2f}", flush=True)
        del dense, quant
        torch.cuda.empty_cache()


def bench_append_store(a):
    nq = nkv = 32
    hd, bs, maxlen, nks = 128, 16, 640, 8
    qkvd = (nq + 2 * nkv) * hd
    torch.manual_seed(0)
    slabs = torch.randn(nks, bs, qkvd, device="cuda")
    pos = torch.arange(maxlen, dtype=torch.float32, device="cuda")
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device="cuda").float() / hd))
    ang = pos[:, None] * inv[None, :]
    cosb, sinb = ang.cos().contiguous(), ang.sin().contiguous()
    lens = torch.full((bs,), maxlen // 2, dtype=torch.int32, device="cuda")
    kc = torch.zeros(bs, maxlen, nkv, hd, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    k8 = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cuda")
    v8 = F.Fp8KVCache.zeros(bs, maxlen, nkv, hd, "cuda")

    def app16(i):
        return C.rope_qkv_decode(slabs, None, kc, vc, lens, cosb, sinb, nq, True)

    def app8(i):
        return C.rope_qkv_decode_fp8(slabs, None, k8.codes, k8.scale, v8.codes,
                                     v8.scale, lens, cosb, sinb, nq, True)

    plen = 128
    total = bs * plen
    qkv = torch.randn(total, qkvd, device="cuda").to(torch.bfloat16)
    _, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    k, v = k.reshape(total, nkv, hd), v.reshape(total, nkv, hd)
    cu = torch.arange(0, total + 1, plen, dtype=torch.int32, device="cuda")
    positions = (torch.arange(total, device="cuda") % plen).long()

    def store16(i):
        seq_id = torch.bucketize(torch.arange(total, device="cuda"),
                                 cu[1:].long(), right=True)
        kc[seq_id, positions] = k
        vc[seq_id, positions] = v

    def store8(i):
        F.fp8_kv_store(k, v, k8, v8, cu, positions)

    print(f"\nappend (slabs nks={nks}, bs={bs}, {nq}/{nkv} heads, hd {hd}) and "
          f"prefill store ({total} tokens), iters={a.iters}")
    print(f"{'':22} {'bf16 us min/med/max':>27} {'fp8 us min/med/max':>27} {'bf16/fp8':>8}")
    for name, f16, f8 in (("decode append", app16, app8),
                          ("prefill store", store16, store8)):
        t16, t8 = [], []
        for _ in range(a.repeats):
            t16.append(window(f16, a.iters, a.iters // 10))
            t8.append(window(f8, a.iters, a.iters // 10))
        s16, s8 = stats(t16), stats(t8)
        print(f"{name:22} {fmt(s16)} {fmt(s8)} {s16[1] / s8[1]:8.2f}", flush=True)


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
    for name, kv, wq in (("bf16", "none", "none"),
                         ("fp8 KV", "fp8_e4m3", "none"),
                         ("fp8 KV + fp8 weights", "fp8_e4m3", "fp8_e4m3")):
        g = GenerationHyperparameters(max_new_tokens=a.ctx_new, greedy=True,
                                      use_hip_graph=True, kv_quant=kv,
                                      weight_quant=wq)
        generate(m, toks, cu, g)
        sessions[name] = m._gen_session[1]  # keeps its graph and buffers
        assert sessions[name].decoder.graph is not None, "no captured graph"
        m._gen_session = None
    torch.cuda.synchronize()

    def cache_bytes(s):
        return sum(c.nbytes() if isinstance(c, F.Fp8KVCache)
                   else c.numel() * c.element_size()
                   for pair in s.kv_caches for c in pair)

    print(f"\n{a.layers}-layer llama-7B-shaped model, bs={bs}, context "
          f"{plen + a.ctx_new}: KV caches {cache_bytes(sessions['bf16']) / 1e9:.3f} GB "
          f"bf16, {cache_bytes(sessions['fp8 KV']) / 1e9:.3f} GB fp8")
    t = {q: [] for q in sessions}
    for _ in range(a.repeats):
        for q, s in sessions.items():
            t[q].append(window(lambda i: s.decoder.graph.replay(),
                               a.step_iters, a.step_iters // 10))
    print(f"{'decode step (graph replay)':28} {'min us':>10} {'med us':>10} {'max us':>10}")
    for q in sessions:
        lo, med, hi = stats(t[q])
        print(f"{q:28} {lo:10.1f} {med:10.1f} {hi:10.1f}")
    base = statistics.median(t["bf16"])
    for q in list(sessions)[1:]:
        print(f"bf16 / {q} (medians): {base / statistics.median(t[q]):.3f}")


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawTextHelpFormatter)
    p.add_argument("--iters", type=int, default=1000,
                   help="launches per window (append and store)")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--rotate-gb", type=float, default=1.0)
    p.add_argument("--only-hd", type=int, default=0)
    p.add_argument("--layers", type=int, default=32)
    p.add_argument("--ctx-new", type=int, default=512,
                   help="generated tokens before the step is timed")
    p.add_argument("--step-iters", type=int, default=100)
    p.add_argument("--skip-attention", action="store_true")
    p.add_argument("--skip-append", action="store_true")
    p.add_argument("--skip-model", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if not a.skip_attention:
        bench_attention(a)
    if not a.skip_append:
        bench_append_store(a)
    if not a.skip_model:
        bench_model(a)
