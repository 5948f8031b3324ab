"""Hot ops: HIP kernels with torch reference fallbacks.

HIP kernels (realhf_amd/ops/csrc/, reference op inventory SURVEY.md §2.2):
  rms_norm           — fused RMSNorm fwd/bwd (reference used TransformerEngine);
                       gemma_style=True is the same kernels in their 1 + w
                       weight mode
  apply_rotary       — RoPE on packed varlen qk (reference: flash-attn fused rotary)
  qk_norm_rope       — per-head QK RMSNorm (qwen3) + RoPE on q and k in one
                       kernel fwd/bwd, reading q/k in place from the QKV
                       GEMM output; REALHF_AMD_NO_QK_NORM_OPS=1 puts the
                       norm back on torch (qk_norm_rope_ref)
  swiglu             — silu(gate)*up fused fwd/bwd
  geglu              — gelu_tanh(gate)*up fused fwd/bwd (gemma), the swiglu
                       kernels with the activation as a template parameter;
                       REALHF_AMD_NO_GEMMA_OPS=1 puts gemma's norm and GeGLU
                       back on torch
  attn_varlen        — flash-attention packed prefill (reference: flash_attn_varlen_func)
  attn_decode        — single-token GQA decode over contiguous KV cache
                       (reference: flash_attn_with_kvcache); both attention
                       ops take softcap (gemma-2's logit soft-cap,
                       cap * tanh(score / cap) before the masks), applied
                       inside the HIP kernels and by every torch route
  gae                — packed GAE scan (reference: realhf._C.cugae)
  slice_intervals /
  set_intervals      — flat-param interval gather/scatter (realhf._C.interval_op_cuda)
  fused_adamw        — flat-buffer AdamW (reference: apex fused adam via Megatron)
  vocab_logprobs     — per-token log-prob over a vocab slice, fwd/bwd without
                       fp32 [tokens, vocab] temporaries (opt-in, see parallel/tp.py)
  quantize_rows_e4m3 — per-row OCP e4m3 weight quantizer (q, scale) for FP8
                       weight-only decode; maybe_skinny_linear /
                       skinny_linear_nc take the pair as fp8=(q, scale) and
                       stream q instead of the bf16 weight
                       (REALHF_AMD_NO_FP8_SKINNY=1: fp8_linear_ref instead)
  Fp8KVCache         — e4m3 KV cache (codes + per-row fp32 scales):
                       fp8_kv_store (quantizing prefill store), the fused
                       decode block's rope_qkv_decode_fp8 append and
                       attn_decode over the pair (attn_decode_fp8);
                       REALHF_AMD_NO_FP8_KV=1 and the CPU take the
                       fp8_kv_*_ref / attn_decode_fp8_ref torch forms

All torch reference paths are fp32-upcast where the reference math is fp32.
"""
import math
import os
from typing import List, Optional, Tuple

import torch

from realhf_amd import ops as _ops

# Head dims the HIP attention kernels (attn_varlen fwd/bwd, attn_decode) are
# instantiated for.  The one gate for every caller: the varlen/decode
# dispatch and the FP8 KV store below, the fused decode block's
# fused_decode_blocker (models/layers.py) and hipGraph decode
# (decode_graph_supported in models/generation.py, parallel/pp.py).
HIP_ATTN_HEAD_DIMS = (64, 128, 256)


def hip_attn_supported(dtype, head_dim: int, device) -> bool:
    """Do the HIP attention kernels take this dtype and head dim on this
    device?  bf16 on a GPU at one of HIP_ATTN_HEAD_DIMS."""
    return (torch.device(device).type == "cuda" and dtype == torch.bfloat16
            and head_dim in HIP_ATTN_HEAD_DIMS)


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
def rms_norm_ref(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps)
    return (out * weight.float()).to(x.dtype)


def gemma_rms_norm_ref(x, weight, eps):
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps)
    return (out * (1.0 + weight.float())).to(x.dtype)


def gemma_ops_enabled() -> bool:
    """Gemma's norm and GeGLU run on the HIP kernels unless
    REALHF_AMD_NO_GEMMA_OPS=1 (read at call time), which restores the torch
    norm and GeGLU and keeps Gemma out of the decode slab fast paths: the
    A/B baseline for tests/test_gemma_ops_gpu.py and tools/bench_gemma_ops.py."""
    return os.environ.get("REALHF_AMD_NO_GEMMA_OPS") != "1"


class _RMSNormFn(torch.autograd.Function):
    """gemma=True scales by 1 + weight (summed in fp32 inside the kernel)."""

    @staticmethod
    def forward(ctx, x, weight, eps, gemma=False):
        C = _ops.require_hip()
        fwd = C.gemma_rmsnorm_fwd if gemma else C.rmsnorm_fwd
        out, rstd = fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, rstd)
        ctx.gemma = gemma
        return out

    @staticmethod
    def backward(ctx, grad_out):
        C = _ops.require_hip()
        x, weight, rstd = ctx.saved_tensors
        bwd = C.gemma_rmsnorm_bwd if ctx.gemma else C.rmsnorm_bwd
        dx, dw = bwd(grad_out.contiguous(), x, weight, rstd)
        return dx, dw, None, None


def rms_norm(x, weight, eps: float = 1e-5, gemma_style: bool = False):
    if _ops.use_hip(x) and (not gemma_style or gemma_ops_enabled()):
        return _RMSNormFn.apply(x.contiguous(), weight, eps, gemma_style)
    if gemma_style:
        return gemma_rms_norm_ref(x, weight, eps)
    return rms_norm_ref(x, weight, eps)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
class RotaryCache:
    """Host-precomputed cos/sin tables (Appendix B: never sinf/cosf on
    device).  Shapes: [max_len, head_dim/2]."""

    def __init__(self):
        self._cache = {}

    def get(
        self,
        head_dim: int,
        max_len: int,
        base: float,
        device,
        dtype=torch.float32,
        scaling: Optional[float] = None,
        scaling_type: Optional[str] = None,
        orig_max_pos: Optional[int] = None,
    ):
        """scaling_type: None/"linear" divide positions by `scaling`
        (position interpolation); "dynamic" rescales `base` NTK-style when
        max_len exceeds orig_max_pos (reference rotary.py:121
        `_update_cos_sin_cache` mirrors HF's dynamic-NTK rule).  Dynamic
        tables are keyed by their exact length — the base depends on it —
        so no doubling growth is applied there."""
        dynamic = scaling_type == "dynamic" and scaling is not None
        if dynamic:
            orig = int(orig_max_pos or max_len)
            max_len = max(int(max_len), orig)
            if max_len > orig:
                base = base * (
                    (scaling * max_len / orig) - (scaling - 1)
                ) ** (head_dim / (head_dim - 2))
            scaling = None  # dynamic rescales base; positions stay unscaled
        key = (head_dim, base, str(device), dtype, scaling)
        cos, sin, cached_len = self._cache.get(key, (None, None, 0))
        if cached_len < max_len:
            if not dynamic:
                max_len = max(max_len, 2 * cached_len, 2048)
            inv_freq = 1.0 / (
                base ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim)
            )
            t = torch.arange(max_len, dtype=torch.float64)
            if scaling is not None:
                t = t / scaling
            freqs = torch.outer(t, inv_freq)
            cos = freqs.cos().to(dtype).to(device)
            sin = freqs.sin().to(dtype).to(device)
            self._cache[key] = (cos, sin, max_len)
        cos, sin, _ = self._cache[key]
        return cos, sin


rotary_cache = RotaryCache()


def apply_rotary_ref(
    x: torch.Tensor,  # [total, n_heads, head_dim]
    cos: torch.Tensor,  # [max_len, head_dim/2]
    sin: torch.Tensor,
    positions: torch.Tensor,  # [total] int32/64
    interleaved: bool = False,
) -> torch.Tensor:
    c = cos[positions].unsqueeze(1)  # [total, 1, hd/2]
    s = sin[positions].unsqueeze(1)
    xf = x.float()
    hd = x.shape[-1]
    if interleaved:
        x1, x2 = xf[..., 0::2], xf[..., 1::2]
        o1 = x1 * c - x2 * s
        o2 = x2 * c + x1 * s
        out = torch.stack([o1, o2], dim=-1).flatten(-2)
    else:
        x1, x2 = xf[..., : hd // 2], xf[..., hd // 2 :]
        o1 = x1 * c - x2 * s
        o2 = x2 * c + x1 * s
        out = torch.cat([o1, o2], dim=-1)
    return out.to(x.dtype)


class _RotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, positions, interleaved):
        C = _ops.require_hip()
        out = C.rope_fwd(x, cos, sin, positions, interleaved, False)
        ctx.save_for_backward(cos, sin, positions)
        ctx.interleaved = interleaved
        return out

    @staticmethod
    def backward(ctx, grad):
        C = _ops.require_hip()
        cos, sin, positions = ctx.saved_tensors
        dx = C.rope_fwd(grad.contiguous(), cos, sin, positions, ctx.interleaved, True)
        return dx, None, None, None, None


def apply_rotary(x, cos, sin, positions, interleaved=False):
    if _ops.use_hip(x):
        return _RotaryFn.apply(x.contiguous(), cos, sin, positions, interleaved)
    return apply_rotary_ref(x, cos, sin, positions, interleaved)


# ---------------------------------------------------------------------------
# Per-head QK RMSNorm + RoPE (qwen3)
# ---------------------------------------------------------------------------
# head dims the fused kernels are instantiated for
QK_NORM_HEAD_DIMS = (64, 128, 256)


def qk_norm_ops_enabled() -> bool:
    """The per-head QK RMSNorm runs inside the HIP kernels (qk_norm_rope,
    rope_qkv_decode_norm) unless REALHF_AMD_NO_QK_NORM_OPS=1 (read at call
    time), which puts the norm back on torch in front of the un-normed
    kernels: the A/B baseline for tests/test_qwen3_gpu.py and
    tools/bench_qk_norm.py."""
    return os.environ.get("REALHF_AMD_NO_QK_NORM_OPS") != "1"


def qk_norm_rope_ref(q, k, q_w, k_w, eps, cos, sin, positions,
                     interleaved=False):
    """fp32 torch: plain-weight RMSNorm over head_dim on every q and k head
    row [total, heads, hd], then apply_rotary_ref (cos None: no rotation)."""

    def one(x, w):
        xf = x.float()
        n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
        if cos is not None:
            n = apply_rotary_ref(n, cos, sin, positions, interleaved)
        return n.to(x.dtype)

    return one(q, q_w), one(k, k_w)


class _QKNormRopeFn(torch.autograd.Function):
    """One launch forward (q and k, norm + RoPE) and one backward; q and k are
    saved as they came, normally views into the QKV GEMM output."""

    @staticmethod
    def forward(ctx, q, k, q_w, k_w, eps, cos, sin, positions):
        C = _ops.require_hip()
        rope = cos is not None
        if not rope:  # unused by the kernels
            cos = sin = positions = q.new_empty(0, dtype=torch.float32)
        q_out, k_out, rstd = C.qk_norm_rope_fwd(q, k, q_w, k_w, eps, cos, sin,
                                                positions, rope)
        ctx.save_for_backward(q, k, q_w, k_w, rstd, cos, sin, positions)
        ctx.rope = rope
        return q_out, k_out

    @staticmethod
    def backward(ctx, dq_out, dk_out):
        C = _ops.require_hip()
        q, k, q_w, k_w, rstd, cos, sin, positions = ctx.saved_tensors
        dq, dk, dqw, dkw = C.qk_norm_rope_bwd(
            dq_out.contiguous(), dk_out.contiguous(), q, k, q_w, k_w, rstd,
            cos, sin, positions, ctx.rope)
        return dq, dk, dqw, dkw, None, None, None, None


def _qk_rows(x):
    """x [total, heads, hd] as the kernels take it: unit stride inside a head
    row and from head to head; the token stride is free."""
    if x.stride(2) == 1 and (x.shape[1] == 1 or x.stride(1) == x.shape[2]) \
            and x.stride(0) % 4 == 0 and x.data_ptr() % 8 == 0:
        return x
    return x.contiguous()


def qk_norm_rope(q, k, q_w, k_w, eps, cos, sin, positions, interleaved=False):
    """q' = rope(rmsnorm_head(q) * q_w), k' likewise with k_w; q [total, nq,
    hd], k [total, nkv, hd], weights [hd], cos = None skips the rotation.  On
    the GPU one HIP kernel forward and one backward, reading q and k in place
    when they are views into the merged QKV output; interleaved rotary, a
    head dim outside QK_NORM_HEAD_DIMS, fp32, the CPU and
    REALHF_AMD_NO_QK_NORM_OPS=1 take qk_norm_rope_ref."""
    if (_ops.use_hip(q) and qk_norm_ops_enabled() and not interleaved
            and q.shape[-1] in QK_NORM_HEAD_DIMS and q.element_size() == 2):
        return _QKNormRopeFn.apply(_qk_rows(q), _qk_rows(k), q_w, k_w, eps,
                                   cos, sin, positions)
    return qk_norm_rope_ref(q, k, q_w, k_w, eps, cos, sin, positions,
                            interleaved)


# ---------------------------------------------------------------------------
# SwiGLU epilogue: silu(gate) * up
# ---------------------------------------------------------------------------
def swiglu_ref(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: [tokens, 2*idim] with gate = [:, :idim], up = [:, idim:]."""
    idim = gate_up.shape[-1] // 2
    gate, up = gate_up[..., :idim], gate_up[..., idim:]
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate_up.dtype)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up):
        C = _ops.require_hip()
        out = C.swiglu_fwd(gate_up)
        ctx.save_for_backward(gate_up)
        return out

    @staticmethod
    def backward(ctx, grad):
        C = _ops.require_hip()
        (gate_up,) = ctx.saved_tensors
        return C.swiglu_bwd(grad.contiguous(), gate_up)


def swiglu(gate_up):
    if _ops.use_hip(gate_up):
        return _SwiGLUFn.apply(gate_up.contiguous())
    return swiglu_ref(gate_up)


# ---------------------------------------------------------------------------
# GeGLU epilogue (gemma): gelu_tanh(gate) * up
# ---------------------------------------------------------------------------
def geglu_ref(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: [tokens, 2*idim] with gate = [:, :idim], up = [:, idim:]."""
    gate, up = gate_up.chunk(2, dim=-1)
    return (
        torch.nn.functional.gelu(gate.float(), approximate="tanh") * up.float()
    ).to(gate_up.dtype)


class _GeGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up):
        C = _ops.require_hip()
        out = C.geglu_fwd(gate_up)
        ctx.save_for_backward(gate_up)
        return out

    @staticmethod
    def backward(ctx, grad):
        C = _ops.require_hip()
        (gate_up,) = ctx.saved_tensors
        return C.geglu_bwd(grad.contiguous(), gate_up)


def geglu(gate_up):
    if (_ops.use_hip(gate_up) and gate_up.element_size() == 2
            and gemma_ops_enabled()):
        return _GeGLUFn.apply(gate_up.contiguous())
    return geglu_ref(gate_up)


# ---------------------------------------------------------------------------
# Attention — packed varlen (prefill/training)
# ---------------------------------------------------------------------------
def _softcap(scores: torch.Tensor, softcap: Optional[float]) -> torch.Tensor:
    """softcap * tanh(scores / softcap) on (unmasked) fp32 scores; None or 0
    is no cap."""
    if not softcap:
        return scores
    return torch.tanh(scores / softcap) * softcap


def attn_varlen_ref(
    q: torch.Tensor,  # [total, nq, hd]
    k: torch.Tensor,  # [total, nkv, hd]
    v: torch.Tensor,  # [total, nkv, hd]
    cu_seqlens: torch.Tensor,  # [bs+1] int32
    causal: bool = True,
    softmax_scale: Optional[float] = None,
    window: Optional[int] = None,  # sliding window incl. self (mistral)
    softcap: Optional[float] = None,  # logit soft-cap (gemma-2); None/0 = off
) -> torch.Tensor:
    """Per-sequence SDPA in fp32 — the numerics oracle.  With softcap the
    scaled scores become softcap * tanh(scores / softcap) before the masks."""
    nq, hd = q.shape[1], q.shape[2]
    nkv = k.shape[1]
    scale = softmax_scale or (1.0 / math.sqrt(hd))
    out = torch.empty_like(q)
    rep = nq // nkv
    cu = cu_seqlens.tolist()
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        qi = q[s:e].transpose(0, 1).float()  # [nq, L, hd]
        ki = k[s:e].transpose(0, 1).float()
        vi = v[s:e].transpose(0, 1).float()
        if rep > 1:
            ki = ki.repeat_interleave(rep, dim=0)
            vi = vi.repeat_interleave(rep, dim=0)
        scores = torch.matmul(qi, ki.transpose(-1, -2)) * scale
        scores = _softcap(scores, softcap)
        L = e - s
        if causal and L > 1:
            mask = torch.triu(
                torch.ones(L, L, dtype=torch.bool, device=q.device), diagonal=1
            )
            scores = scores.masked_fill(mask, float("-inf"))
        if window is not None and L > window:
            # visible keys for query i: (i - window, i]  (HF mistral mask)
            wmask = torch.tril(
                torch.ones(L, L, dtype=torch.bool, device=q.device),
                diagonal=-window,
            )
            scores = scores.masked_fill(wmask, float("-inf"))
        probs = torch.softmax(scores, dim=-1)
        o = torch.matmul(probs, vi)  # [nq, L, hd]
        out[s:e] = o.transpose(0, 1).to(q.dtype)
    return out


def _attn_varlen_blocked_torch(q, k, v, cu_seqlens, causal, scale, window=None,
                               softcap=None):
    """Batched-padded torch implementation on GPU (used for backward
    recompute until the hand-written HIP backward lands): one set of
    batched rocBLAS GEMMs instead of a per-sequence python loop (the loop
    was CPU-launch-bound: bs x layers x ~15 kernels)."""
    total, nq, hd = q.shape
    nkv = k.shape[1]
    rep = nq // nkv
    lens = (cu_seqlens[1:] - cu_seqlens[:-1]).long()
    bs = lens.shape[0]
    Lmax = int(lens.max())
    device = q.device
    pos = torch.arange(total, device=device)
    seq_id = torch.bucketize(pos, cu_seqlens[1:].long(), right=True)
    local = pos - cu_seqlens[:-1].long()[seq_id]

    # bf16 MFMA matmuls (fp32 accumulation inside rocBLAS) with fp32
    # softmax — the same numerics class as a flash-attention backward;
    # fp32 matmuls here would run at 1/16 of the bf16 MFMA rate.
    mm_dtype = torch.bfloat16 if q.is_cuda else torch.float32

    def pad(x, nh):
        xp = x.new_zeros(bs, Lmax, nh, hd)
        xp[seq_id, local] = x
        return xp.permute(0, 2, 1, 3).to(mm_dtype)  # [bs, nh, Lmax, hd]

    qp = pad(q, nq)
    kp = pad(k, nkv)
    vp = pad(v, nkv)
    if rep > 1:
        kp = kp.repeat_interleave(rep, dim=1)
        vp = vp.repeat_interleave(rep, dim=1)
    scores = torch.matmul(qp * scale, kp.transpose(-1, -2)).float()
    scores = _softcap(scores, softcap)
    kpos = torch.arange(Lmax, device=device)
    valid = kpos.unsqueeze(0) < lens.unsqueeze(1)  # [bs, Lmax]
    mask = valid.unsqueeze(1).unsqueeze(2)  # [bs,1,1,L]
    if causal:
        cm = kpos.unsqueeze(0) <= kpos.unsqueeze(1)  # [Lq, Lk]
        if window is not None:
            cm = cm & (kpos.unsqueeze(0) > kpos.unsqueeze(1) - window)
        mask = mask & cm.unsqueeze(0).unsqueeze(0)
    scores = scores.masked_fill(~mask, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.nan_to_num(probs, nan=0.0)
    op = torch.matmul(probs.to(mm_dtype), vp)  # [bs, nh, Lmax, hd]
    op = op.permute(0, 2, 1, 3)  # [bs, Lmax, nh, hd]
    return op[seq_id, local].to(q.dtype)


def _check_softcap(softcap: Optional[float]) -> Optional[float]:
    """None for no cap (None or 0), else the positive float."""
    if not softcap:
        return None
    if softcap < 0:
        raise ValueError(f"softcap must be positive, got {softcap}")
    return float(softcap)


class _AttnVarlenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, max_seqlen, causal, scale,
                window=None, softcap=None):
        C = _ops.require_hip()
        out, lse = C.attn_varlen_fwd(q, k, v, cu_seqlens, int(max_seqlen),
                                     causal, scale, int(window or 0),
                                     float(softcap or 0.0))
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens)
        ctx.causal, ctx.scale, ctx.max_seqlen = causal, scale, max_seqlen
        ctx.window = window
        ctx.softcap = softcap
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse, cu_seqlens = ctx.saved_tensors
        if os.environ.get("REALHF_AMD_NO_HIP_ATTN_BWD") != "1":
            # hand-written MFMA backward (attn_bwd.hip): kv-stationary,
            # dQ via fp32 atomics, per-q-head dK/dV reduced here for GQA;
            # REALHF_AMD_ATTN_BWD_DET=1 (opt-in; bench.py sets it) sums dQ
            # from per-kv-block partials in block order instead, which is
            # bit-reproducible but allocates ceil(max_seqlen/64) dQ-sized
            # fp32 slots per call;
            # sliding-window via key-range restriction like the forward.
            # In-context A/B: 3.51 vs 3.19 samples/s over the padded
            # recompute fallback (REALHF_AMD_NO_HIP_ATTN_BWD=1).
            C = _ops.require_hip()
            dout = grad_out.contiguous()
            dsum = (dout.float() * out.float()).sum(-1)  # [total, nq]
            dq32, dk32, dv32 = C.attn_varlen_bwd(
                q, k, v, dout, lse, dsum, cu_seqlens, ctx.causal, ctx.scale,
                int(ctx.window or 0),
                int(ctx.max_seqlen)
                if os.environ.get("REALHF_AMD_ATTN_BWD_DET") == "1" else 0,
                float(ctx.softcap or 0.0),
            )
            nq, nkv = q.shape[1], k.shape[1]
            rep = nq // nkv
            if rep > 1:
                t = dk32.shape[0]
                dk32 = dk32.view(t, nkv, rep, -1).sum(2)
                dv32 = dv32.view(t, nkv, rep, -1).sum(2)
            return (dq32.to(q.dtype), dk32.to(k.dtype), dv32.to(v.dtype),
                    None, None, None, None, None, None)
        # Fallback: blocked recompute with rocBLAS GEMMs (fp32 softmax).
        with torch.enable_grad():
            qg = q.detach().requires_grad_(True)
            kg = k.detach().requires_grad_(True)
            vg = v.detach().requires_grad_(True)
            ref = _attn_varlen_blocked_torch(
                qg, kg, vg, cu_seqlens, ctx.causal, ctx.scale,
                window=ctx.window, softcap=ctx.softcap,
            )
            dq, dk, dv = torch.autograd.grad(ref, (qg, kg, vg), grad_out)
        return dq, dk, dv, None, None, None, None, None, None


def attn_varlen(q, k, v, cu_seqlens, max_seqlen, causal=True, softmax_scale=None,
                window=None, softcap: Optional[float] = None):
    """softcap: attention logit soft-cap (gemma-2), applied by every route
    to the scaled scores before the masks; None or 0 is no cap."""
    scale = softmax_scale or (1.0 / math.sqrt(q.shape[-1]))
    softcap = _check_softcap(softcap)
    if window is not None and window >= int(max_seqlen):
        window = None  # window wider than any sequence: plain causal
    if (
        _ops.use_hip(q)
        and hip_attn_supported(q.dtype, q.shape[-1], q.device)
        and (window is None or causal)
    ):
        return _AttnVarlenFn.apply(
            q.contiguous(), k.contiguous(), v.contiguous(),
            cu_seqlens, max_seqlen, causal, scale, window, softcap,
        )
    if q.is_cuda:
        # odd head dims / dtypes / binding sliding window: batched rocBLAS
        # path (still GPU)
        return _attn_varlen_blocked_torch(q, k, v, cu_seqlens, causal, scale,
                                          window=window, softcap=softcap)
    return attn_varlen_ref(q, k, v, cu_seqlens, causal, scale, window=window,
                           softcap=softcap)


# ---------------------------------------------------------------------------
# Attention — single-token decode over contiguous KV cache
# ---------------------------------------------------------------------------
def attn_decode_ref(
    q: torch.Tensor,  # [bs, nq, hd] — the new token's q
    k_cache: torch.Tensor,  # [bs, max_len, nkv, hd]
    v_cache: torch.Tensor,
    cache_seqlens: torch.Tensor,  # [bs] int32 — valid length INCLUDING new token
    softmax_scale: Optional[float] = None,
    window: Optional[int] = None,
    softcap: Optional[float] = None,
) -> torch.Tensor:
    bs, nq, hd = q.shape
    nkv = k_cache.shape[2]
    rep = nq // nkv
    scale = softmax_scale or (1.0 / math.sqrt(hd))
    out = torch.empty_like(q)
    for b in range(bs):
        L = int(cache_seqlens[b])
        lo = max(0, L - window) if window is not None else 0
        kb = k_cache[b, lo:L].transpose(0, 1).float()  # [nkv, L-lo, hd]
        vb = v_cache[b, lo:L].transpose(0, 1).float()
        if rep > 1:
            kb = kb.repeat_interleave(rep, dim=0)
            vb = vb.repeat_interleave(rep, dim=0)
        qb = q[b].unsqueeze(1).float()  # [nq, 1, hd]
        scores = torch.matmul(qb, kb.transpose(-1, -2)) * scale
        scores = _softcap(scores, softcap)
        probs = torch.softmax(scores, dim=-1)
        out[b] = torch.matmul(probs, vb).squeeze(1).to(q.dtype)
    return out


def attn_decode(q, k_cache, v_cache, cache_seqlens, softmax_scale=None,
                window=None, softcap: Optional[float] = None):
    scale = softmax_scale or (1.0 / math.sqrt(q.shape[-1]))
    softcap = _check_softcap(softcap)
    if window is not None and k_cache.shape[1] <= window:
        window = None  # cache can never exceed the window: plain causal
    hip = (
        _ops.use_hip(q)
        and hip_attn_supported(q.dtype, q.shape[-1], q.device)
        and q.shape[1] // k_cache.shape[2] in (1, 2, 4, 8)
    )
    if isinstance(k_cache, Fp8KVCache):
        if hip and fp8_kv_enabled():
            C = _ops.require_hip()
            return C.attn_decode_fp8(q, k_cache.codes, k_cache.scale,
                                     v_cache.codes, v_cache.scale,
                                     cache_seqlens, scale, int(window or 0),
                                     softcap or 0.0)
        return attn_decode_fp8_ref(q, k_cache, v_cache, cache_seqlens, scale,
                                   window=window, softcap=softcap)
    if hip:
        C = _ops.require_hip()
        return C.attn_decode(q, k_cache, v_cache, cache_seqlens, scale,
                             int(window or 0), softcap or 0.0)
    return attn_decode_ref(q, k_cache, v_cache, cache_seqlens, scale,
                           window=window, softcap=softcap)


# ---------------------------------------------------------------------------
# GAE over packed sequences
# ---------------------------------------------------------------------------
def gae_ref(
    rewards: torch.Tensor,  # [total] fp32 — per-token rewards (shifted: len-1 per seq)
    values: torch.Tensor,  # [total + bs] fp32 — values with one extra bootstrap per seq
    cu_seqlens: torch.Tensor,  # [bs+1] — over the REWARD lengths
    bootstrap: torch.Tensor,  # [bs] bool — whether the last value bootstraps
    gamma: float,
    lam: float,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """advantages [total], returns [total].  Mirrors cugae1d_nolp_misalign
    (reference csrc/cugae/gae.cu:10): values for sequence i live at
    [cu[i]+i, cu[i+1]+i+1) — one longer than rewards."""
    adv = torch.zeros_like(rewards)
    ret = torch.zeros_like(rewards)
    cu = cu_seqlens.tolist()
    bs = len(cu) - 1
    for i in range(bs):
        rs, re = cu[i], cu[i + 1]
        vs = rs + i
        lastgae = 0.0
        L = re - rs
        for t in range(L - 1, -1, -1):
            nex = values[vs + t + 1]
            if t == L - 1 and not bool(bootstrap[i]):
                nex = values.new_zeros(())
            delta = rewards[rs + t] + gamma * nex - values[vs + t]
            lastgae = delta + gamma * lam * lastgae
            adv[rs + t] = lastgae
            ret[rs + t] = lastgae + values[vs + t]
    return adv, ret


def gae(rewards, values, cu_seqlens, bootstrap, gamma, lam):
    if _ops.use_hip(rewards):
        C = _ops.require_hip()
        return C.gae_1d(rewards, values, cu_seqlens, bootstrap, float(gamma), float(lam))
    return gae_ref(rewards, values, cu_seqlens, bootstrap, gamma, lam)


# ---------------------------------------------------------------------------
# Vocab log-probs: per-row (target logit, max, sum-exp) over a vocab slice
# ---------------------------------------------------------------------------
def vocab_logprob_stats_ref(
    logits: torch.Tensor,  # [n, v_local]
    labels: torch.Tensor,  # [n] int64 global vocab ids
    vocab_start: int = 0,
    ignore_index: int = -100,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(target, rowmax, sumexp), all fp32 [n], over the local vocab slice:
    rowmax = max_j x, sumexp = sum_j exp(x - rowmax), target = the raw logit
    at column label - vocab_start if that lies in the slice, else 0.  An
    all -inf slice gives (rowmax, sumexp) = (-inf, 0); ignored rows give
    (0, 0, 1)."""
    x = logits.float()
    v_local = x.shape[-1]
    rowmax = x.max(dim=-1).values
    finite_max = torch.where(torch.isinf(rowmax) & (rowmax < 0),
                             torch.zeros_like(rowmax), rowmax)
    sumexp = (x - finite_max.unsqueeze(-1)).exp().sum(dim=-1)
    local = labels - vocab_start
    in_range = (local >= 0) & (local < v_local)
    safe = local.clamp(0, v_local - 1)
    target = x.gather(-1, safe.unsqueeze(-1)).squeeze(-1)
    target = torch.where(in_range, target, torch.zeros_like(target))
    ign = labels == ignore_index
    target = target.masked_fill(ign, 0.0)
    rowmax = rowmax.masked_fill(ign, 0.0)
    sumexp = sumexp.masked_fill(ign, 1.0)
    return target, rowmax, sumexp


def vocab_logprob_bwd_ref(logits, labels, lse, grad_out, vocab_start=0,
                          ignore_index=-100):
    """dlogits = grad_out * (onehot(label - vocab_start) - exp(x - lse)) in
    fp32, cast to logits.dtype; ignored rows are zero."""
    v_local = logits.shape[-1]
    g = (logits.float() - lse.unsqueeze(-1)).exp_().mul_(-grad_out.unsqueeze(-1))
    local = labels - vocab_start
    in_range = (local >= 0) & (local < v_local) & (labels != ignore_index)
    safe = local.clamp(0, v_local - 1)
    add = torch.where(in_range, grad_out, torch.zeros_like(grad_out))
    g.scatter_add_(-1, safe.unsqueeze(-1), add.unsqueeze(-1))
    g.masked_fill_((labels == ignore_index).unsqueeze(-1), 0.0)
    return g.to(logits.dtype)


def combine_vocab_stats(target, rowmax, sumexp, group=None):
    """Merge per-slice statistics into (logp, lse).  group=None is the
    single-rank case; with a group, three [n]-vector all-reduces (max, sum,
    sum) merge the TP ranks' vocab slices."""
    import torch.distributed as dist

    g = rowmax.clone()
    if group is not None:
        dist.all_reduce(g, op=dist.ReduceOp.MAX, group=group)
    # an all -inf slice has sumexp == 0 and possibly rowmax == g == -inf
    factor = torch.where(sumexp == 0, torch.zeros_like(sumexp),
                         (rowmax - g).exp())
    se = sumexp * factor
    t = target.clone()
    if group is not None:
        dist.all_reduce(se, group=group)
        dist.all_reduce(t, group=group)
    lse = g + se.log()
    return t - lse, lse


def _vocab_logprob_hip(logits: torch.Tensor) -> bool:
    return _ops.use_hip(logits) and logits.dtype in (torch.bfloat16,
                                                      torch.float32)


class _VocabLogProbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, vocab_start, group, ignore_index):
        if _vocab_logprob_hip(logits):
            C = _ops.require_hip()
            logits = logits.contiguous()
            labels = labels.contiguous()
            stats = C.vocab_logprob_fwd(logits, labels, vocab_start,
                                        ignore_index)
        else:
            stats = vocab_logprob_stats_ref(logits, labels, vocab_start,
                                            ignore_index)
        logp, lse = combine_vocab_stats(*stats, group=group)
        logp = logp.masked_fill(labels == ignore_index, 0.0)
        ctx.save_for_backward(logits, labels, lse)
        ctx.vocab_start, ctx.ignore_index = vocab_start, ignore_index
        return logp

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, lse = ctx.saved_tensors
        grad_out = grad_out.float().contiguous()
        if _vocab_logprob_hip(logits):
            C = _ops.require_hip()
            dlogits = C.vocab_logprob_bwd(logits, labels, lse, grad_out,
                                          ctx.vocab_start, ctx.ignore_index)
        else:
            dlogits = vocab_logprob_bwd_ref(logits, labels, lse, grad_out,
                                            ctx.vocab_start, ctx.ignore_index)
        return dlogits, None, None, None, None


def vocab_logprobs(logits, labels, *, vocab_start=0, group=None,
                   ignore_index=-100):
    """fp32 log p(label) per row of [n, v_local] logits whose columns are
    the vocab slice starting at vocab_start; rows labelled ignore_index
    give 0 and a zero gradient.  Saves only the logits, the labels and the
    [n] log-sum-exp for backward."""
    return _VocabLogProbFn.apply(logits, labels.long(), int(vocab_start), group,
                                 int(ignore_index))


# ---------------------------------------------------------------------------
# Flat-parameter interval gather/scatter
# ---------------------------------------------------------------------------
def slice_intervals_ref(src: torch.Tensor, intervals: torch.Tensor) -> torch.Tensor:
    outs = [src[s:e] for s, e in intervals.tolist()]
    return torch.cat(outs) if outs else src.new_empty(0)


def set_intervals_ref(src: torch.Tensor, dst: torch.Tensor, intervals: torch.Tensor):
    off = 0
    for s, e in intervals.tolist():
        n = e - s
        dst[s:e] = src[off : off + n]
        off += n
    return dst


def slice_intervals(src, intervals):
    if _ops.use_hip(src) and intervals.shape[0] >= 128:
        C = _ops.require_hip()
        return C.slice_intervals(src, intervals.to(src.device))
    return slice_intervals_ref(src, intervals)


def set_intervals(src, dst, intervals):
    if _ops.use_hip(dst) and intervals.shape[0] >= 128:
        C = _ops.require_hip()
        C.set_intervals(src, dst, intervals.to(dst.device))
        return dst
    return set_intervals_ref(src, dst, intervals)


def merge_intervals(intervals: List[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """Coalesce adjacent/overlapping [a,b) pairs (reference:
    csrc/interval_op/interval_op.cpp merge_intervals)."""
    if not intervals:
        return []
    intervals = sorted(intervals)
    out = [list(intervals[0])]
    for s, e in intervals[1:]:
        if s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [tuple(x) for x in out]


# ---------------------------------------------------------------------------
# Weight-streaming skinny GEMM (decode M <= 16); wins on square-ish
# projections (o/down: ~1.6-2x over hipBLASLt), loses on very wide N —
# callers pick per shape (tools/bench_skinny.py is the A/B harness).
# ---------------------------------------------------------------------------
def _sg_kslice_max() -> int:
    """Max K elements per split-K slice (tunes workgroup count); A/B via
    REALHF_AMD_SG_KSLICE, default 1024."""
    global _SG_KSLICE
    if _SG_KSLICE is None:
        _SG_KSLICE = int(os.environ.get("REALHF_AMD_SG_KSLICE", 1024))
    return _SG_KSLICE


_SG_KSLICE = None


def skinny_splitk(K: int) -> int:
    """The split-K factor of the skinny GEMMs: 8, doubled while a K slice
    would be longer than _sg_kslice_max()."""
    splitk = 8
    while K // splitk > _sg_kslice_max():
        splitk *= 2
    return splitk


def _skinny_plan(x: torch.Tensor, w: torch.Tensor, fp8):
    """What maybe_skinny_linear and skinny_linear_nc share: None where the
    skinny kernels do not take x @ w^T (w: the e4m3 codes when there is an
    fp8 pair, which also asks for K % 64 == 0), else (extension, split-K
    factor, shared fp32 workspace)."""
    if not (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and not torch.is_grad_enabled()
        and x.dim() == 2
        and x.shape[0] <= 16
        and x.stride(1) == 1
        and x.stride(0) == x.shape[1]
        and w.stride(1) == 1
        and w.shape[0] % 64 == 0
        and w.shape[1] % (32 if fp8 is None else 64) == 0
        and (fp8 is None or fp8_skinny_enabled())
        and _ops.hip_available()
    ):
        return None
    from realhf_amd.base.constants import get_global_memory_buffer

    splitk = skinny_splitk(x.shape[1])
    ws = get_global_memory_buffer().get_tensor(
        (2 * splitk * 16 * w.shape[0],), torch.float32, "skinny_gemm_ws"
    )
    return _ops.require_hip(), splitk, ws


def maybe_skinny_linear(x: torch.Tensor, w: torch.Tensor,
                        residual: Optional[torch.Tensor] = None,
                        fp8: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                        ) -> Optional[torch.Tensor]:
    """x @ w^T (+ residual, folded into the combine) on the skinny kernel,
    None where _skinny_plan does not take it.  fp8 = (q, scale) from
    quantize_rows_e4m3(w): stream the e4m3 codes instead of w
    (skinny_gemm_fp8).  With a pair the result is never None: whatever the
    kernel does not take (CPU, M > 16, REALHF_AMD_NO_FP8_SKINNY=1) goes through
    fp8_linear_ref, so the weights in use are the quantized ones either way."""
    if fp8 is not None:
        w = fp8[0]
    # in-context the weight-streaming kernel also edges out hipBLASLt on the
    # wide-N shapes (A/B: 3.09 vs 3.05 samples/s); opt out with
    # REALHF_AMD_NO_SKINNY_WIDE=1
    wide_ok = (w.shape[0] <= 2 * w.shape[1]
               or os.environ.get("REALHF_AMD_NO_SKINNY_WIDE") != "1")
    plan = _skinny_plan(x, w, fp8) if wide_ok else None
    if plan is None:
        if fp8 is not None:
            return fp8_linear_ref(x, fp8[0], fp8[1], residual)
        return None
    C, splitk, ws = plan
    if residual is not None:
        residual = residual.contiguous()
    if fp8 is not None:
        return C.skinny_gemm_fp8(x, fp8[0], fp8[1], ws, splitk, residual)
    if os.environ.get("REALHF_AMD_SKINNY_V2") == "1":
        # v2 (in-launch semaphore combine) measured SLOWER at every decode
        # shape: the per-block agent-scope release (buffer_wbl2) does not
        # amortize at 1.5k-2.7k blocks (qkv 67us vs 22.8us at splitk 8).
        # Kept for reference / small-grid experiments only.
        return C.skinny_gemm2(x, w, ws, _skinny_sem(x.device), splitk, residual)
    return C.skinny_gemm(x, w, ws, splitk, residual)


def skinny_linear_nc(x: torch.Tensor, w: torch.Tensor,
                     fp8: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                     ) -> Optional[torch.Tensor]:
    """Like maybe_skinny_linear but WITHOUT the split-K combine: returns
    the fp32 partial slabs [nks, M, N], to be summed in the CONSUMING
    kernel's prologue (launch-boundary reduce: rope_qkv_decode /
    add_rmsnorm_fwd / swiglu_fwd all accept slabs).  The slabs live in the
    shared skinny workspace — consume them before the next skinny call.
    fp8 = (q, scale): the slabs come from skinny_gemm_fp8_nc, row scale
    already applied; None where _skinny_plan does not take it (the caller
    then goes on to maybe_skinny_linear with the same pair)."""
    if fp8 is not None:
        w = fp8[0]
    plan = _skinny_plan(x, w, fp8)
    if plan is None:
        return None
    C, splitk, ws = plan
    if fp8 is not None:
        return C.skinny_gemm_fp8_nc(x, fp8[0], fp8[1], ws, splitk)
    return C.skinny_gemm_nc(x, w, ws, splitk)


_SKINNY_SEM: dict = {}


def _skinny_sem(device) -> torch.Tensor:
    """Per-device split-K semaphore buffer (one int32 per n-tile; 1024
    covers N up to 65536).  Zeroed ONCE at allocation; the kernel leaves
    every counter back at zero."""
    t = _SKINNY_SEM.get(device)
    if t is None:
        t = torch.zeros(1024, dtype=torch.int32, device=device)
        _SKINNY_SEM[device] = t
    return t


# ---------------------------------------------------------------------------
# FP8 weight-only decode: per-row e4m3 quantizer and its linear reference
# ---------------------------------------------------------------------------
E4M3_MAX = 448.0


def quantize_rows_e4m3_ref(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q [N, K] float8_e4m3fn, scale [N] fp32) with scale = amax / 448 per
    row (1 for an all-zero row) and q = rne_e4m3(float(w) / scale).  The
    fixed definition the HIP quantizer matches bit for bit.  Rows with
    non-finite weights get no special handling."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / E4M3_MAX)
    return (wf / scale[:, None]).to(torch.float8_e4m3fn), scale


def quantize_rows_e4m3(w: torch.Tensor, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantize bf16 w [N, K] (stride(1) == 1, any row stride) per row.
    out = (q, scale) writes into caller-owned buffers (stable addresses for
    a captured graph) and returns them."""
    if _ops.use_hip(w):
        C = _ops.require_hip()
        if out is None:
            q, scale = C.quantize_rows_e4m3(w)
            return q, scale
        C.quantize_rows_e4m3_(w, out[0], out[1])
        return out
    q, scale = quantize_rows_e4m3_ref(w)
    if out is None:
        return q, scale
    out[0].copy_(q)
    out[1].copy_(scale)
    return out


def fp8_skinny_enabled() -> bool:
    """(q, scale) weights run on skinny_gemm_fp8 unless
    REALHF_AMD_NO_FP8_SKINNY=1 (read at call time), which sends the same
    pair through fp8_linear_ref: the A/B baseline and the oracle of
    tests/test_fp8_decode_gpu.py."""
    return os.environ.get("REALHF_AMD_NO_FP8_SKINNY") != "1"


def fp8_linear_ref(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor,
                   residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x @ (q * scale[:, None])^T (+ residual) in fp32, returned in x.dtype."""
    out = x.float() @ (q.float() * scale[:, None]).t()
    if residual is not None:
        out = out + residual.float()
    return out.to(x.dtype)


# ---------------------------------------------------------------------------
# FP8 KV cache: e4m3 codes + one fp32 scale per head row
# ---------------------------------------------------------------------------
class Fp8KVCache:
    """One layer's K (or V) cache in e4m3: codes [bs, maxlen, nkv, hd]
    float8_e4m3fn and one fp32 scale per (sequence, kv head, position) laid
    out [bs, nkv, maxlen] (the decode kernel's lane = key reads are
    contiguous).  A row is quantize_rows_e4m3_ref of the hd bf16 values the
    bf16 cache would hold.  .shape is the codes' shape, so callers that only
    ask a cache for its sizes take either kind."""

    __slots__ = ("codes", "scale")

    def __init__(self, codes: torch.Tensor, scale: torch.Tensor):
        bs, maxlen, nkv, _ = codes.shape
        assert codes.dtype == torch.float8_e4m3fn
        assert scale.dtype == torch.float32 and scale.shape == (bs, nkv, maxlen)
        self.codes = codes
        self.scale = scale

    @classmethod
    def zeros(cls, bs, maxlen, nkv, hd, device):
        """Code 0 decodes to 0: a zeroed cache is an all-zero cache."""
        return cls(
            torch.zeros(bs, maxlen, nkv, hd, dtype=torch.uint8,
                        device=device).view(torch.float8_e4m3fn),
            torch.zeros(bs, nkv, maxlen, dtype=torch.float32, device=device),
        )

    @property
    def shape(self):
        return self.codes.shape

    @property
    def device(self):
        return self.codes.device

    def nbytes(self) -> int:
        return self.codes.numel() + 4 * self.scale.numel()

    def dequantize(self) -> torch.Tensor:
        """fp32 [bs, maxlen, nkv, hd]"""
        return self.codes.float() * self.scale.transpose(1, 2).unsqueeze(-1)


def fp8_kv_enabled() -> bool:
    """An FP8 KV cache is written and read by the HIP kernels unless
    REALHF_AMD_NO_FP8_KV=1 (read at call time), which sends the same cache
    through the torch references: the A/B baseline and the oracle of
    tests/test_fp8_kv_gpu.py."""
    return os.environ.get("REALHF_AMD_NO_FP8_KV") != "1"


def _fp8_kv_put(cache: Fp8KVCache, x: torch.Tensor, seq: torch.Tensor,
                pos: torch.Tensor):
    """Quantize head rows x [n, nkv, hd] (from their bf16 rounding) into
    cache at (seq[i], pos[i])."""
    n, nkv, hd = x.shape
    # quantize_rows_e4m3: the reference on the CPU; on the GPU the row
    # quantizer kernel, which is bit for bit that reference (torch's own GPU
    # division is not the correctly rounded one the definition asks for)
    q, s = quantize_rows_e4m3(
        x.detach().to(torch.bfloat16).reshape(-1, hd).contiguous())
    # index_put on uint8 views: float8 tensors do not take it everywhere
    cache.codes.view(torch.uint8)[seq, pos] = q.view(torch.uint8).reshape(n, nkv, hd)
    cache.scale[seq, :, pos] = s.reshape(n, nkv)


def fp8_kv_append_ref(k, v, k_cache: Fp8KVCache, v_cache: Fp8KVCache,
                      cache_seqlens):
    """Decode append: k / v [bs, nkv, hd] (K after RoPE) go to position
    cache_seqlens - 1 of their sequence."""
    idx = (cache_seqlens.long() - 1).clamp(min=0)
    b_idx = torch.arange(k.shape[0], device=k.device)
    _fp8_kv_put(k_cache, k, b_idx, idx)
    _fp8_kv_put(v_cache, v, b_idx, idx)


def fp8_kv_store_ref(k, v, k_cache: Fp8KVCache, v_cache: Fp8KVCache,
                     cu_seqlens, positions):
    """Prefill store: packed k / v [total, nkv, hd] go to (sequence of the
    token, positions[token])."""
    seq_id = torch.bucketize(
        torch.arange(k.shape[0], device=k.device), cu_seqlens[1:].long(),
        right=True,
    )
    _fp8_kv_put(k_cache, k, seq_id, positions.long())
    _fp8_kv_put(v_cache, v, seq_id, positions.long())


def fp8_kv_store(k, v, k_cache: Fp8KVCache, v_cache: Fp8KVCache, cu_seqlens,
                 positions):
    """Quantizing prefill store: one HIP kernel for bf16 K/V on the GPU, the
    reference elsewhere and under REALHF_AMD_NO_FP8_KV=1."""
    if (
        _ops.use_hip(k)
        and fp8_kv_enabled()
        and hip_attn_supported(k.dtype, k.shape[-1], k.device)
    ):
        C = _ops.require_hip()

        def rows(x):  # [total, nkv, hd] views into the QKV projection pass
            x = x.detach()
            ok = (x.stride(2) == 1
                  and (x.shape[1] == 1 or x.stride(1) == x.shape[2])
                  and (x.shape[0] <= 1 or x.stride(0) % 8 == 0)
                  and x.data_ptr() % 16 == 0)
            return x if ok else x.contiguous()

        C.kv_store_fp8(rows(k), rows(v), k_cache.codes, k_cache.scale,
                       v_cache.codes, v_cache.scale,
                       cu_seqlens.to(torch.int32).contiguous(),
                       positions.long().contiguous())
        return
    fp8_kv_store_ref(k, v, k_cache, v_cache, cu_seqlens, positions)


def attn_decode_fp8_ref(q, k_cache: Fp8KVCache, v_cache: Fp8KVCache,
                        cache_seqlens, softmax_scale=None, window=None,
                        softcap=None):
    """attn_decode_ref in fp32 on the dequantized caches, returned in
    q.dtype.  Only the attended positions [lo, L) are dequantized, so
    whatever lies outside them (stale or non-finite) never enters."""
    bs, nq, hd = q.shape
    scale = softmax_scale or (1.0 / math.sqrt(hd))
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    for b in range(bs):
        L = int(cache_seqlens[b])
        lo = max(0, L - window) if window is not None else 0

        def deq(c):
            x = c.codes[b:b + 1, lo:L].float()
            return x * c.scale[b:b + 1, :, lo:L].transpose(1, 2).unsqueeze(-1)

        out[b] = attn_decode_ref(
            q[b:b + 1].float(), deq(k_cache), deq(v_cache),
            torch.tensor([L - lo]), scale, softcap=softcap)[0]
    return out.to(q.dtype)


# ---------------------------------------------------------------------------
# Fused AdamW on flat buffers
# ---------------------------------------------------------------------------
def fused_adamw_ref(
    param_f32: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step: int,
    bf16_out: Optional[torch.Tensor] = None,
    grad_scale: float = 1.0,
):
    g = grad.float() * grad_scale
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    param_f32.mul_(1 - lr * weight_decay)
    param_f32.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if bf16_out is not None:
        bf16_out.copy_(param_f32)
    return param_f32


def fused_adamw(param_f32, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                weight_decay, step, bf16_out=None, grad_scale=1.0):
    if _ops.use_hip(param_f32):
        C = _ops.require_hip()
        C.fused_adamw(
            param_f32, grad, exp_avg, exp_avg_sq,
            bf16_out if bf16_out is not None else param_f32.new_empty(0).to(torch.bfloat16),
            float(lr), float(beta1), float(beta2), float(eps),
            float(weight_decay), int(step), float(grad_scale),
            bf16_out is not None,
        )
        return param_f32
    return fused_adamw_ref(
        param_f32, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
        weight_decay, step, bf16_out, grad_scale,
    )
