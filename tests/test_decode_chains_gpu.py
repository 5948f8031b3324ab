"""Decode kernels after the load batching: slab consumers, few-row norms and
the skinny GEMM pipeline give bit for bit what the sequential forms give.

Slab consumers are fed synthetic fp32 slabs [nks, rows, N] and compared with
a sequential fp32 sum on the GPU in slab order (slab 0, +1, +2, ...), then the
op's own definition.  The slabs are built so that any other order, or a batch
padded with zero slabs, changes bits:
  * column 0 is -0.0 in every slab (and in the residual): its sum is -0.0, and
    -0.0 + 0.0 would be +0.0;
  * with nks >= 3 every other element carries (+1e8, +1, -1e8) in three slabs
    chosen per element, in that order: sequentially the 1 is absorbed (the ulp
    of 1e8 is 8), in any order that cancels 1e8 first it survives.
Bit equality is checked on the integer view of the tensors, which unlike
torch.equal also tells -0.0 from +0.0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs GPU", allow_module_level=True)

from realhf_amd.ops import functional as F  # noqa: E402
import realhf_amd._C as C  # noqa: E402

NKS = [1, 2, 7, 8, 9, 16, 17]
ROWS = [1, 3, 16]
ROW_GATE = 16  # RMS_ROW_MAX_ROWS in rmsnorm.hip
H_GATE = 8192  # 256 threads * 8 elements * RMS_ROW_MAX_NP

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def bits_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    it = _INT[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def seq_sum(slabs):
    acc = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        acc = acc + slabs[s]
    return acc


_SLABS = {}


def make_slabs(nks, rows, N):
    """[nks, rows, N] fp32 on the GPU and its sequential sum; cached, shared
    between tests and never modified."""
    key = (nks, rows, N)
    if key not in _SLABS:
        g = torch.Generator(device="cuda").manual_seed(1000 * nks + 10 * rows + N)
        s = torch.randn(nks, rows, N, generator=g, device="cuda") * 0.5
        if nks >= 3:
            order = torch.rand(nks, rows, N, generator=g, device="cuda").argsort(0)
            abc = order[:3].sort(0).values
            for i, val in enumerate((1e8, 1.0, -1e8)):
                s.scatter_add_(0, abc[i:i + 1], torch.full_like(s[:1], val))
        s[:, :, 0] = -0.0
        _SLABS[key] = (s, seq_sum(s))
    return _SLABS[key]


def test_slab_inputs_are_order_sensitive():
    """The fixture does what the docstring says (not a kernel test)."""
    s, ref = make_slabs(9, 3, 64)
    assert bits_equal(ref[:, 0], torch.full_like(ref[:, 0], -0.0))
    assert not bits_equal(ref, s.flip(0).contiguous().sum(0))
    assert not bits_equal(ref, seq_sum(s.flip(0).contiguous()))
    padded = seq_sum(torch.cat([s, torch.zeros_like(s[:1])]))
    assert not bits_equal(ref, padded)


# ---------------------------------------------------------------------------
# slab add + rmsnorm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [264, 2048, 4096, H_GATE + 8])
@pytest.mark.parametrize("gemma", [False, True])
def test_add_rmsnorm_slabs(gemma, H):
    fwd = C.gemma_add_rmsnorm_fwd if gemma else C.add_rmsnorm_fwd
    norm_ref = F.gemma_rms_norm_ref if gemma else F.rms_norm_ref
    g = torch.Generator(device="cuda").manual_seed(H)
    w = torch.randn(H, generator=g, device="cuda").to(torch.bfloat16)
    for rows in ROWS:
        resid = (torch.randn(rows, H, generator=g, device="cuda") * 0.5
                 ).to(torch.bfloat16)
        resid[:, 0] = -0.0
        for nks in NKS:
            slabs, ssum = make_slabs(nks, rows, H)
            out, sum_out = fwd(slabs, resid, w, 1e-5)
            want = (ssum + resid.float()).to(torch.bfloat16)
            what = f"H{H} rows{rows} nks{nks} gemma={gemma}"
            assert torch.equal(sum_out, want), what
            assert bits_equal(sum_out, want), what
            # the bound of test_ops_gpu.test_rmsnorm_fwd_bwd
            ref = norm_ref(want.float(), w.float(), 1e-5)
            torch.testing.assert_close(out.float(), ref, atol=5e-2, rtol=5e-2,
                                       msg=lambda m: f"{what}: {m}")


# ---------------------------------------------------------------------------
# swiglu / geglu
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("I", [64, 1376])
@pytest.mark.parametrize("gelu", [False, True])
def test_glu_slabs(gelu, I):
    fwd = C.geglu_fwd if gelu else C.swiglu_fwd
    op = F.geglu if gelu else F.swiglu
    for rows in ROWS:
        for nks in NKS:
            slabs, ssum = make_slabs(nks, rows, 2 * I)
            got = fwd(slabs)
            what = f"I{I} rows{rows} nks{nks} gelu={gelu}"
            # the same fp32 sum as one slab: isolates the batching
            one = fwd(ssum[None].contiguous())
            assert torch.equal(got, one), what
            assert bits_equal(got, one), what
            # the op on the bf16 of the sum, bounds of test_swiglu_fwd_bwd
            with torch.no_grad():
                ref = op(ssum.to(torch.bfloat16))
            torch.testing.assert_close(got.float(), ref.float(), atol=3e-2,
                                       rtol=3e-2, msg=lambda m: f"{what}: {m}")


# ---------------------------------------------------------------------------
# rope_qkv_decode / rope_qkv_decode_fp8
# ---------------------------------------------------------------------------
def _rope_tables(maxlen, hd):
    pos = torch.arange(maxlen, device="cuda", dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device="cuda").float() / hd))
    ang = pos[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _lens(bs, maxlen):
    return [(1, maxlen, 5)[i % 3] for i in range(bs)]


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qkv_decode_slabs(hd, use_bias):
    nq, nkv, maxlen = 2, 1, 8
    qkvd = (nq + 2 * nkv) * hd
    cosb, sinb = _rope_tables(maxlen, hd)
    g = torch.Generator(device="cuda").manual_seed(hd)
    bias = (torch.randn(qkvd, generator=g, device="cuda") * 0.5
            ).to(torch.bfloat16) if use_bias else None
    for bs in ROWS:
        lens = _lens(bs, maxlen)
        cs = torch.tensor(lens, dtype=torch.int32, device="cuda")
        fill = torch.randn(bs, maxlen, nkv, hd, generator=g, device="cuda"
                           ).to(torch.bfloat16)
        written = torch.zeros(bs, maxlen, dtype=torch.bool, device="cuda")
        written[torch.arange(bs), torch.tensor(lens) - 1] = True
        for nks in NKS:
            slabs, ssum = make_slabs(nks, bs, qkvd)
            what = f"hd{hd} bias={use_bias} bs{bs} nks{nks}"
            kc1, vc1, kc2, vc2 = (fill.clone() for _ in range(4))
            q1 = C.rope_qkv_decode(ssum[None].contiguous(), bias, kc1, vc1, cs,
                                   cosb, sinb, nq, True)
            q2 = C.rope_qkv_decode(slabs, bias, kc2, vc2, cs, cosb, sinb, nq,
                                   True)
            assert torch.equal(q2, q1) and bits_equal(q2, q1), what
            for a, b in ((kc2, kc1), (vc2, vc1)):
                assert torch.equal(a, b) and bits_equal(a, b), what
                assert bits_equal(a[~written], fill[~written]), what
                assert not bits_equal(a[written], fill[written]), what


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qkv_decode_fp8_slabs(hd, use_bias):
    nq, nkv, maxlen = 2, 1, 8
    qkvd = (nq + 2 * nkv) * hd
    cosb, sinb = _rope_tables(maxlen, hd)
    g = torch.Generator(device="cuda").manual_seed(hd + 1)
    bias = (torch.randn(qkvd, generator=g, device="cuda") * 0.5
            ).to(torch.bfloat16) if use_bias else None

    def filled(bs):
        codes = torch.randint(0, 0x78, (bs, maxlen, nkv, hd), generator=g,
                              device="cuda", dtype=torch.uint8)
        scale = torch.rand(bs, nkv, maxlen, generator=g, device="cuda") + 0.5
        return codes, scale

    for bs in ROWS:
        lens = _lens(bs, maxlen)
        cs = torch.tensor(lens, dtype=torch.int32, device="cuda")
        kfill, vfill = filled(bs), filled(bs)
        written = torch.zeros(bs, maxlen, dtype=torch.bool, device="cuda")
        written[torch.arange(bs), torch.tensor(lens) - 1] = True
        for nks in NKS:
            slabs, ssum = make_slabs(nks, bs, qkvd)
            what = f"fp8 hd{hd} bias={use_bias} bs{bs} nks{nks}"
            res = []
            for qkv in (ssum[None].contiguous(), slabs):
                kc, ks = kfill[0].clone(), kfill[1].clone()
                vc, vs = vfill[0].clone(), vfill[1].clone()
                q = C.rope_qkv_decode_fp8(
                    qkv, bias, kc.view(torch.float8_e4m3fn), ks,
                    vc.view(torch.float8_e4m3fn), vs, cs, cosb, sinb, nq, True)
                res.append((q, kc, ks, vc, vs))
            for a, b in zip(res[1], res[0]):
                assert torch.equal(a, b) and bits_equal(a, b), what
            _, kc, ks, vc, vs = res[1]
            for codes, scale, (fc, fs) in ((kc, ks, kfill), (vc, vs, vfill)):
                assert bits_equal(codes[~written], fc[~written]), what
                sw = written[:, None, :].expand_as(scale)
                assert bits_equal(scale[~sw], fs[~sw]), what
                assert not bits_equal(scale[sw], fs[sw]), what


# ---------------------------------------------------------------------------
# combine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nks", [1, 7, 8, 9, 16, 17])
def test_combine_is_sequential_sum(nks):
    """K = 64 * nks with splitk = nks gives kslice 64 and nks slabs (K 1088
    with splitk 17 ...).  x rows carry a large pair that cancels across
    slices, so the slab sum is order sensitive."""
    K, N = 64 * nks, 192
    g = torch.Generator(device="cuda").manual_seed(nks)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    for M in (1, 5, 16):
        x = (torch.randn(M, K, generator=g, device="cuda") * 0.5)
        if nks >= 3:  # +big in slice 0, -big in the last slice, same w column
            x[:, 0] = 16384.0
            x[:, K - 64] = -16384.0
            w[:, K - 64] = w[:, 0]
        x = x.to(torch.bfloat16)
        res = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16)
        ws = torch.empty(nks * 16 * N, dtype=torch.float32, device="cuda")
        slabs = C.skinny_gemm_nc(x, w, ws, nks).clone()
        assert slabs.shape == (nks, M, N)
        ssum = seq_sum(slabs)
        for r in (None, res):
            got = C.skinny_gemm(x, w, ws, nks, r)
            want = (ssum if r is None else ssum + r.float()).to(torch.bfloat16)
            assert torch.equal(got, want), f"nks{nks} M{M} resid={r is not None}"
            assert bits_equal(got, want), f"nks{nks} M{M} resid={r is not None}"


# ---------------------------------------------------------------------------
# few-row norm: the register kernel against the row-loop kernel, same rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16,
                                   torch.float32])
@pytest.mark.parametrize("H", [264, 4096, H_GATE + 8])
@pytest.mark.parametrize("gemma", [False, True])
def test_rmsnorm_rows_across_gate(gemma, H, dtype):
    """rows in {1, 16, gate, gate + 1} (the gate is 16 rows): the same 16 rows
    alone (register kernel when H fits) and as the first 16 of gate + 1 rows
    (row-loop kernel) give the same out and rstd bit for bit.  fp32 has no
    register kernel: for it both calls run the row loop."""
    fwd = C.gemma_rmsnorm_fwd if gemma else C.rmsnorm_fwd
    norm_ref = F.gemma_rms_norm_ref if gemma else F.rms_norm_ref
    g = torch.Generator(device="cuda").manual_seed(H + gemma)
    x = torch.randn(ROW_GATE + 1, H, generator=g, device="cuda").to(dtype)
    w = torch.randn(H, generator=g, device="cuda").to(dtype)
    out_big, rstd_big = fwd(x, w, 1e-5)
    ref = norm_ref(x.float(), w.float(), 1e-5)
    torch.testing.assert_close(out_big.float(), ref, atol=5e-2, rtol=5e-2)
    for rows in (1, ROW_GATE):
        out, rstd = fwd(x[:rows].contiguous(), w, 1e-5)
        what = f"H{H} rows{rows} gemma={gemma} {dtype}"
        torch.testing.assert_close(out.float(), ref[:rows], atol=5e-2,
                                   rtol=5e-2, msg=lambda m: f"{what}: {m}")
        assert bits_equal(out, out_big[:rows]), what
        assert bits_equal(rstd, rstd_big[:rows]), what


@pytest.mark.parametrize("H", [264, 4096, H_GATE + 8])
@pytest.mark.parametrize("gemma", [False, True])
def test_add_rmsnorm_rows_across_gate(gemma, H):
    """The RESID mode (bf16 x + residual) likewise: out and sum_out."""
    fwd = C.gemma_add_rmsnorm_fwd if gemma else C.add_rmsnorm_fwd
    g = torch.Generator(device="cuda").manual_seed(H + 2 + gemma)
    x = torch.randn(ROW_GATE + 1, H, generator=g, device="cuda").to(torch.bfloat16)
    r = torch.randn(ROW_GATE + 1, H, generator=g, device="cuda").to(torch.bfloat16)
    w = torch.randn(H, generator=g, device="cuda").to(torch.bfloat16)
    out_big, sum_big = fwd(x, r, w, 1e-5)
    assert bits_equal(sum_big, (x.float() + r.float()).to(torch.bfloat16))
    for rows in (1, ROW_GATE):
        out, s = fwd(x[:rows].contiguous(), r[:rows].contiguous(), w, 1e-5)
        what = f"H{H} rows{rows} gemma={gemma}"
        assert bits_equal(s, sum_big[:rows]), what
        assert bits_equal(out, out_big[:rows]), what


# ---------------------------------------------------------------------------
# skinny GEMM slabs, bf16 and fp8 weights
# ---------------------------------------------------------------------------
# (K, splitk): splitk as skinny_splitk picks it, plus a forced one whose last
# slice is partial (704 / 4 -> kslice 192, slices 192, 192, 192, 128).  K
# 11008 already has a partial last slice (16 x 704, the last 448).
K_BF16 = [32, 96, 128, 160, 704, 11008]
# the fp8 kernel takes K % 64 == 0 only and its batch is 4 x 64 deep: the
# members of the list above it accepts, plus its own no-full-batch (64, 192)
# and batch-plus-tail (320) sizes
K_FP8 = [64, 128, 192, 320, 704, 11008]


# further (K, splitk), by what the pipeline does with the slice (bf16 batch
# 128 / fp8 batch 256): an even and an odd number of full batches with and
# without a tail, a last slice with no full batch, and a slice longer than the
# 1024 columns whose x tile is staged from registers (8192 / 4 -> 2048)
K_MORE = [(2048, 8), (2304, 8), (4096, 8), (1792, 4), (6144, 8), (8192, 8),
          (8192, 4)]


def _k_cases(ks):
    return [(K, F.skinny_splitk(K)) for K in ks] + [(704, 4)] + K_MORE


def _check_slabs(fp8, M, N, K, splitk):
    g = torch.Generator(device="cuda").manual_seed(K + N + M)
    x = (torch.randn(M, K, generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    kslice = (K // splitk + 63) // 64 * 64
    nks = (K + kslice - 1) // kslice
    ws = torch.empty(nks * 16 * N, dtype=torch.float32, device="cuda")
    if fp8:
        q, scale = C.quantize_rows_e4m3(w)
        wf = q.float() * scale[:, None]
        run = lambda xx: C.skinny_gemm_fp8_nc(xx, q, scale, ws, splitk).clone()
    else:
        wf = w.float()
        run = lambda xx: C.skinny_gemm_nc(xx, w, ws, splitk).clone()
    what = f"fp8={fp8} M{M} N{N} K{K} splitk{splitk}"
    a = run(x)
    assert a.shape == (nks, M, N), what
    for s in range(nks):
        lo, hi = s * kslice, min(K, (s + 1) * kslice)
        ref = x[:, lo:hi].float() @ wf[:, lo:hi].t()
        # the bound of test_skinny_gemm_with_residual / test_fp8_gemm_matches_ref
        torch.testing.assert_close(a[s], ref, atol=0.3, rtol=3e-2,
                                   msg=lambda m: f"{what} slab {s}: {m}")
    assert bits_equal(a, run(x)), what
    xpad = torch.zeros(16, K, dtype=torch.bfloat16, device="cuda")
    xpad[:M] = x
    assert bits_equal(a, run(xpad)[:, :M].contiguous()), what


@pytest.mark.parametrize("K,splitk", _k_cases(K_BF16))
def test_skinny_gemm_slabs(K, splitk):
    for M in (1, 5, 16):
        for N in (64, 192):
            _check_slabs(False, M, N, K, splitk)


@pytest.mark.parametrize("K,splitk", _k_cases(K_FP8))
def test_skinny_gemm_fp8_slabs(K, splitk):
    for M in (1, 5, 16):
        for N in (64, 192):
            _check_slabs(True, M, N, K, splitk)
