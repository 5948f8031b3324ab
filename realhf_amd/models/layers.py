"""Transformer layer modules over flat-buffer parameter views.

Reference semantics: realhf/impl/model/nn/real_llm_base.py (ReaLModelBlock:103,
VocabPositionEmbedding:260, OutputHead:346, SequenceParallelCriticHead:356,
ParallelActorHead:370) and modules/{attn,mlp}.py.

Every module receives its parameters as a dict of tensors that are VIEWS
into the owning ReaLModel's contiguous flat buffer; modules never allocate
weights.  TP behavior comes from the current model scope's grid
(realhf_amd.base.constants); with tp_size == 1 every collective is a no-op
so the same code runs single-process on CPU.

MI355X specifics: wq/wk/wv (and gate/up) flat regions are adjacent, so the
module runs ONE hipBLASLt GEMM over the concatenated view; RMSNorm (plain
and gemma's 1 + w) / RoPE / SwiGLU / GeGLU / attention are the hand-written
HIP kernels in realhf_amd.ops.

ReaLModelBlock.forward dispatches over three routes: training/prefill and
eager decode attention, which share the wo + MLP epilogue, and the fused
decode block, which runs exactly when fused_decode_blocker() names no reason
(generation's quant blockers are built on the same function).  Every decode
projection goes down one ladder, _decode_linear().
"""
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from realhf_amd.api.model import ReaLModelConfig
from realhf_amd.base import constants
from realhf_amd.ops import functional as ops
from realhf_amd.ops import require_hip
from realhf_amd.parallel import cp as cp_mod
from realhf_amd.parallel import mappings


def _maybe_merged(params: Dict[str, torch.Tensor], names, dim_out_total):
    """If the named 2-D params are contiguous consecutive views of the flat
    buffer, return a single merged [sum_out, in] view; else None."""
    ts = [params[n] for n in names]
    base = ts[0]
    if any(t.dtype != base.dtype or t.device != base.device for t in ts):
        return None
    try:
        storages = {t.untyped_storage().data_ptr() for t in ts}
    except RuntimeError:
        return None
    if len(storages) != 1:
        return None
    off = base.storage_offset()
    for t in ts:
        if t.storage_offset() != off or not t.is_contiguous():
            return None
        off += t.numel()
    in_dim = base.shape[1]
    merged = base.as_strided((dim_out_total, in_dim), (in_dim, 1), base.storage_offset())
    return merged


def _linear(x, w, b=None):
    return F.linear(x, w, b)


def _decode_linear(x, w, fp8=None, slabs=False,
                   residual=None) -> Tuple[torch.Tensor, str]:
    """The decode step's projection ladder for x @ w^T, fp8 = the block's
    (q, scale) pair of w if it has one.  Returns (result, kind): "slabs",
    ops.skinny_linear_nc's split-K partials, tried only if the caller's next
    kernel sums them (slabs=True); "folded", ops.maybe_skinny_linear with
    `residual` added in its combine; "plain", the same without a residual
    or the dense GEMM, which leaves a residual to the caller.  Outside a
    decode step (grad enabled, M > 16, CPU) a pair-less call is that GEMM."""
    if slabs:
        parts = ops.skinny_linear_nc(x, w, fp8=fp8)
        if parts is not None:
            return parts, "slabs"
    out = ops.maybe_skinny_linear(x, w, residual=residual, fp8=fp8)
    if out is None:
        return _linear(x, w), "plain"
    return out, "plain" if residual is None else "folded"


def fused_decode_blocker(cfg: ReaLModelConfig, dtype, is_cuda: bool,
                         has_lora: bool) -> Optional[str]:
    """Why a decode step does not run the fused decode block (None if it
    does).  The one gate: ReaLModelBlock.forward asks with its run-time
    values, generation's weight_quant / kv_quant blockers for the model."""
    if has_lora:  # adapters are applied in the eager route
        return "LoRA adapters are attached"
    if cfg.qk_layernorm:
        return "qk_layernorm"
    if cfg.head_dim not in ops.HIP_ATTN_HEAD_DIMS:
        return f"head_dim {cfg.head_dim} not in {ops.HIP_ATTN_HEAD_DIMS}"
    if dtype != torch.bfloat16:
        return f"model dtype {dtype} is not bfloat16"
    if os.environ.get("REALHF_AMD_NO_FUSED_DECODE") == "1":
        return "REALHF_AMD_NO_FUSED_DECODE=1"
    if not is_cuda:
        return "the model is not on the GPU"
    return None


class VocabEmbedding(nn.Module):
    """Vocab-parallel token embedding (+ optional learned positions).

    TP: each rank holds rows [r*V/tp, (r+1)*V/tp); out-of-range ids embed
    to zero and the partial results all-reduce over the TP group
    (reference: model_parallel/modules.py:53 ParallelEmbedding)."""

    def __init__(self, cfg: ReaLModelConfig, params: Dict[str, torch.Tensor]):
        super().__init__()
        self.cfg = cfg
        self.wte = params["0.wte.weight"]
        self.wpe = params.get("0.wpe.weight")

    def forward(self, packed_input_ids: torch.Tensor, positions: torch.Tensor):
        tp = constants.tp_world_size() if constants.has_current() else 1
        if tp > 1:
            r = constants.tp_rank()
            n = self.wte.shape[0]
            lo, hi = r * n, (r + 1) * n
            mask = (packed_input_ids >= lo) & (packed_input_ids < hi)
            local_ids = (packed_input_ids - lo).clamp(0, n - 1)
            h = F.embedding(local_ids, self.wte)
            h = h * mask.unsqueeze(-1).to(h.dtype)
            h = mappings.reduce_from_tp_region(h)
        else:
            h = F.embedding(packed_input_ids, self.wte)
        if self.cfg.embedding_multiplier is not None:
            h = h * self.cfg.embedding_multiplier
        if self.wpe is not None:
            h = h + F.embedding(positions, self.wpe)
        if constants.has_current() and constants.sequence_parallel():
            h = mappings.scatter_to_sp_region(h)
        return h


def _norm(cfg: ReaLModelConfig, x, w, b):
    if cfg.norm_type == "rms":
        return ops.rms_norm(x, w, cfg.layer_norm_epsilon)
    if cfg.norm_type == "gemma_rms":
        return ops.rms_norm(x, w, cfg.layer_norm_epsilon, gemma_style=True)
    return F.layer_norm(
        x.float(), (x.shape[-1],), w.float(), b.float() if b is not None else None,
        cfg.layer_norm_epsilon,
    ).to(x.dtype)


class ReaLModelBlock(nn.Module):
    """Pre-LN transformer block on packed sequences (reference:
    real_llm_base.py:103, modules/attn.py:31, modules/mlp.py)."""

    def __init__(self, cfg: ReaLModelConfig, layer_idx: int, params: Dict[str, torch.Tensor], tp_size: int = 1, ep_rank: int = 0, ep_size: int = 1):
        super().__init__()
        self.cfg = cfg
        self.i = layer_idx
        self.p = params
        self.tp_size = tp_size
        self.nq = cfg.n_heads // tp_size
        self.nkv = max(cfg.n_kv_heads // tp_size, 1)
        assert cfg.n_kv_heads % tp_size == 0 or tp_size % cfg.n_kv_heads == 0
        self.hd = cfg.head_dim
        # this block's sliding window (gemma-2 alternates; None = full) and
        # attention logit soft-cap
        self.window = cfg.layer_window(layer_idx)
        self.softcap = cfg.attn_logit_softcap
        i = layer_idx
        self._qkv_names = [f"{i}.attn.wq.weight", f"{i}.attn.wk.weight", f"{i}.attn.wv.weight"]
        self._gu_names = (
            [f"{i}.mlp.gate.weight", f"{i}.mlp.up.weight"]
            if cfg.activation in ("silu", "geglu") and cfg.moe is None
            else None
        )
        self.moe = None
        if cfg.moe is not None:
            from realhf_amd.models.moe import MoELayer

            self.moe = MoELayer(cfg, layer_idx, params, tp_size,
                                ep_rank=ep_rank, ep_size=ep_size)
        # LoRA adapters (injected by ReaLModel.attach_lora): short key
        # ("wq"/"wk"/"wv"/"wo") -> (A [r, in], B [out, r]) views
        self.lora: Dict[str, tuple] = {}
        self.lora_scale = 0.0
        # FP8 weight-only decode: "qkv" / "wo" / "gu" / "down" -> (q, scale)
        # of that projection, installed by the generation session for the
        # span of one generate() call and read by decode steps only
        self.fp8: Dict[str, tuple] = {}

    def decode_weights(self) -> Dict[str, torch.Tensor]:
        """The decode step's projection weights as the fused decode block
        reads them (merged QKV and gate/up views where the flat layout
        gives them); MoE expert weights are not among them."""
        i = self.i
        out = {}
        qkv = _maybe_merged(self.p, self._qkv_names,
                            (self.nq + 2 * self.nkv) * self.hd)
        if qkv is not None:
            out["qkv"] = qkv
        out["wo"] = self.p[f"{i}.attn.wo.weight"]
        if self.moe is None:
            if self._gu_names is not None:
                idim_local = self.p[f"{i}.mlp.gate.weight"].shape[0]
                gu = _maybe_merged(self.p, self._gu_names, 2 * idim_local)
                if gu is not None:
                    out["gu"] = gu
            out["down"] = self.p[f"{i}.mlp.down.weight"]
        return out

    def _lora_delta(self, x, short: str):
        a, b = self.lora[short]
        return ((x @ a.t()) @ b.t()) * self.lora_scale

    # -- attention --------------------------------------------------------
    def _qkv(self, x, fused_sp=None, fp8=None):
        qkv_dim = (self.nq + 2 * self.nkv) * self.hd
        merged = _maybe_merged(self.p, self._qkv_names, qkv_dim)
        if fp8 is not None and merged is not None:
            qkv = ops.maybe_skinny_linear(x, merged, fp8=fp8)
        elif fused_sp is not None and merged is not None:
            # x is PRE-mapping: the fused fn applies (copy|SP-gather) in
            # forward and overlaps the bwd grad collective with the
            # weight-grad GEMM (mappings._ColumnParallelLinear)
            qkv = mappings.column_parallel_linear(x, merged, fused_sp)
        elif merged is not None:
            qkv = _linear(x, merged)
        else:
            if fused_sp is not None:
                x = (mappings.gather_from_sp_region(x) if fused_sp
                     else mappings.copy_to_tp_region(x))
            qkv = torch.cat([_linear(x, self.p[n]) for n in self._qkv_names], dim=-1)
        i = self.i
        if f"{i}.attn.wq.bias" in self.p:
            bias = torch.cat(
                [self.p[f"{i}.attn.w{c}.bias"] for c in "qkv"], dim=0
            )
            qkv = qkv + bias
        q, k, v = qkv.split(
            [self.nq * self.hd, self.nkv * self.hd, self.nkv * self.hd], dim=-1
        )
        if self.lora:
            if "wq" in self.lora:
                q = q + self._lora_delta(x, "wq")
            if "wk" in self.lora:
                k = k + self._lora_delta(x, "wk")
            if "wv" in self.lora:
                v = v + self._lora_delta(x, "wv")
        t = qkv.shape[0]  # with fused SP, x is the pre-gather shard
        return (
            q.reshape(t, self.nq, self.hd),
            k.reshape(t, self.nkv, self.hd),
            v.reshape(t, self.nkv, self.hd),
        )

    def forward(
        self,
        x: torch.Tensor,  # [total, h]
        cu_seqlens: torch.Tensor,
        max_seqlen: int,
        positions: torch.Tensor,  # [total]
        k_cache: Optional[torch.Tensor] = None,  # [bs, maxlen, nkv, hd]
        v_cache: Optional[torch.Tensor] = None,
        cache_seqlens: Optional[torch.Tensor] = None,  # [bs]
        decode: bool = False,
    ):
        """Shared prologue (attention norm, SP/TP input mapping, scale), then
        one route: training/prefill attention, the fused decode block where
        fused_decode_blocker names no reason, else eager decode attention.
        A cache is a bf16 tensor or (kv_quant="fp8_e4m3") an ops.Fp8KVCache."""
        i = self.i
        cfg = self.cfg
        h = _norm(cfg, x, self.p[f"{i}.attn.ln.weight"], self.p.get(f"{i}.attn.ln.bias"))
        sp = constants.has_current() and constants.sequence_parallel()
        # fused column linear (async bwd comm) takes the PRE-mapping h;
        # decode/no-grad/LoRA keep the explicit mapping route
        fused_col = (self.tp_size > 1 and torch.is_grad_enabled()
                     and not self.lora and not decode)
        if not fused_col:
            h = (mappings.gather_from_sp_region(h) if sp
                 else mappings.copy_to_tp_region(h))

        scale = cfg.softmax_scale
        if cfg.scale_attn_by_inverse_layer_idx:
            scale = scale / float(self.i)

        if not decode:
            attn_out = self._prefill_attn(
                h, sp if fused_col else None, scale, cu_seqlens, max_seqlen,
                positions, k_cache, v_cache)
        elif fused_decode_blocker(cfg, h.dtype, h.is_cuda,
                                  bool(self.lora)) is None:
            return self._fused_decode(x, h, sp, scale, k_cache, v_cache,
                                      cache_seqlens)
        else:
            attn_out = self._decode_attn(h, scale, positions, k_cache,
                                         v_cache, cache_seqlens)
        # prefill and training never read the quantized weights
        return self._attn_epilogue(x, attn_out, sp,
                                   self.fp8 if decode else {})

    def _rope_tables(self, rot_len: int, device):
        cfg = self.cfg
        return ops.rotary_cache.get(
            self.hd, rot_len, cfg.rotary_base, device,
            scaling=cfg.rotary_scaling,
            scaling_type=cfg.rotary_scaling_type,
            orig_max_pos=cfg.max_position_embeddings,
        )

    def _qk_ln(self):
        """The per-head QK norm weights (qwen3), [hd] each."""
        i = self.i
        return (self.p[f"{i}.attn.q_ln.weight"],
                self.p[f"{i}.attn.k_ln.weight"])

    def _rope(self, q, k, rot_len: int, positions):
        """q and k as attention takes them: RoPE, behind the per-head QK
        norm where the config has one (one kernel for both)."""
        cfg = self.cfg
        cos = sin = None
        if cfg.apply_rotary:
            cos, sin = self._rope_tables(rot_len, q.device)
        interleaved = cfg.rotary_interleaved
        if cfg.qk_rmsnorm:
            return ops.qk_norm_rope(q, k, *self._qk_ln(),
                                    cfg.layer_norm_epsilon, cos, sin,
                                    positions, interleaved)
        return (ops.apply_rotary(q, cos, sin, positions, interleaved),
                ops.apply_rotary(k, cos, sin, positions, interleaved))

    def _prefill_attn(self, h, fused_sp, scale, cu_seqlens, max_seqlen,
                      positions, k_cache, v_cache):
        """Training and generation prefill: packed varlen attention (through
        the CP all-to-all route under context parallelism), writing the
        prompt K/V into the caches when there are any."""
        cfg = self.cfg
        q, k, v = self._qkv(h, fused_sp=fused_sp)
        if cfg.apply_rotary or cfg.qk_rmsnorm:
            # graph-capture-safe length bound: never read positions back
            if k_cache is not None:
                # generation prefill: use the SESSION's cache length so
                # dynamic-NTK picks one base for prefill AND decode (a
                # per-length base would rotate cached K with a different
                # basis than the decode queries reading it)
                ms = int(k_cache.shape[1])
            elif max_seqlen is not None:
                ms = int(max_seqlen)
            else:  # CP: token shard with explicit positions
                c = cp_mod.current()
                ms = int(c.info.full_max if c is not None
                         else cfg.max_position_embeddings)
            q, k = self._rope(q, k, max(ms, cfg.max_position_embeddings),
                              positions)

        cpctx = cp_mod.current()
        if cpctx is not None:
            # Ulysses context parallelism: tokens are sharded over the CP
            # group; one all-to-all gives this rank ALL tokens for 1/cp of
            # the heads, the varlen kernel runs on full sequences, and a
            # second all-to-all restores the (token-shard, all-heads)
            # layout (parallel/cp.py).
            assert k_cache is None, "CP: no KV-cache prefill/generation"
            assert q.shape[1] % cpctx.size == 0, (
                f"q heads {q.shape[1]} not divisible by cp {cpctx.size}")
            assert k.shape[1] % cpctx.size == 0, (
                f"kv heads {k.shape[1]} not divisible by cp {cpctx.size}")
            q = cp_mod.seq_gather_head_scatter(q)
            k = cp_mod.seq_gather_head_scatter(k)
            v = cp_mod.seq_gather_head_scatter(v)
            attn_out = ops.attn_varlen(
                q, k, v, cpctx.info.full_cu, cpctx.info.full_max,
                causal=True, softmax_scale=scale, window=self.window,
                softcap=self.softcap)
            return cp_mod.head_gather_seq_scatter(attn_out)
        if isinstance(k_cache, ops.Fp8KVCache):
            # prefill into an FP8 cache: one quantizing store; the
            # attention below still sees the fresh bf16 K/V
            ops.fp8_kv_store(k, v, k_cache, v_cache, cu_seqlens, positions)
        elif k_cache is not None:
            # prefill: write all tokens into the cache
            seq_id = torch.bucketize(
                torch.arange(k.shape[0], device=k.device),
                cu_seqlens[1:].long(), right=True)
            k_cache[seq_id, positions] = k.detach().to(k_cache.dtype)
            v_cache[seq_id, positions] = v.detach().to(v_cache.dtype)
        return ops.attn_varlen(
            q, k, v, cu_seqlens, max_seqlen, causal=True,
            softmax_scale=scale, window=self.window, softcap=self.softcap,
        )

    def _decode_attn(self, h, scale, positions, k_cache, v_cache,
                     cache_seqlens):
        """Eager decode, the route of every decode step the fused block does
        not take: one new token per sequence, appended to the cache through
        torch, then ops.attn_decode."""
        cfg = self.cfg
        q, k, v = self._qkv(h, fp8=self.fp8.get("qkv"))
        if cfg.apply_rotary or cfg.qk_rmsnorm:
            # graph-capture-safe length bound: never read positions back
            q, k = self._rope(q, k, int(k_cache.shape[1]), positions)
        bs = k_cache.shape[0]
        assert q.shape[0] == bs
        if isinstance(k_cache, ops.Fp8KVCache):
            ops.fp8_kv_append_ref(k, v, k_cache, v_cache, cache_seqlens)
        else:
            idx = (cache_seqlens.long() - 1).clamp(min=0)
            b_idx = torch.arange(bs, device=q.device)
            k_cache[b_idx, idx] = k.to(k_cache.dtype)
            v_cache[b_idx, idx] = v.to(v_cache.dtype)
        return ops.attn_decode(q, k_cache, v_cache, cache_seqlens, scale,
                               window=self.window, softcap=self.softcap)

    def _attn_epilogue(self, x, attn_out, sp, fp8):
        """wo (+ LoRA delta), SP/TP reduce, bias, (post norm,) residual, MLP:
        the tail of the two non-fused routes."""
        i = self.i
        cfg = self.cfg
        attn_out = attn_out.reshape(attn_out.shape[0], self.nq * self.hd)
        wo = self.p[f"{i}.attn.wo.weight"]
        if "wo" in fp8:
            o = ops.maybe_skinny_linear(attn_out, wo, fp8=fp8["wo"])
        else:
            o = _linear(attn_out, wo)
        if "wo" in self.lora:
            o = o + self._lora_delta(attn_out, "wo")
        o = (mappings.reduce_scatter_to_sp_region(o) if sp
             else mappings.reduce_from_tp_region(o))
        if f"{i}.attn.wo.bias" in self.p:
            o = o + self.p[f"{i}.attn.wo.bias"]
        if cfg.post_norms:  # after the TP reduce: the norm needs whole rows
            o = _norm(cfg, o, self.p[f"{i}.attn.post_ln.weight"], None)
        return self._mlp(x + o, sp, fp8=fp8)

    def _rope_append(self, C, qkv_raw, bias, k_cache, v_cache, cache_seqlens):
        """The fused decode epilogue, one kernel for qkv-split + bias + RoPE
        + KV append: returns q [bs, nq, hd] and writes the new K/V rows at
        cache_seqlens - 1.  qkv_raw is bf16 or split-K slabs."""
        cfg = self.cfg
        cos, sin = self._rope_tables(int(k_cache.shape[1]), qkv_raw.device)
        tail = (cache_seqlens, cos, sin, self.nq, cfg.apply_rotary)
        bf16_form, fp8_form = C.rope_qkv_decode, C.rope_qkv_decode_fp8
        if cfg.qk_rmsnorm and ops.qk_norm_ops_enabled():
            # qwen3: the same launch with the per-head QK norm between the
            # bias add and RoPE
            bf16_form, fp8_form = (C.rope_qkv_decode_norm,
                                   C.rope_qkv_decode_fp8_norm)
            tail += (*self._qk_ln(), cfg.layer_norm_epsilon)
        elif cfg.qk_rmsnorm:
            # REALHF_AMD_NO_QK_NORM_OPS=1, the A/B baseline and test oracle:
            # qkv_raw is bf16 here (_fused_decode asks for no slabs); bias
            # and the norm of the q and k head rows in torch, then the
            # un-normed epilogue
            if bias is not None:
                qkv_raw, bias = qkv_raw + bias, None
            nqk = self.nq + self.nkv
            rows = qkv_raw.reshape(qkv_raw.shape[0], -1, self.hd)
            q_w, k_w = self._qk_ln()
            w = torch.cat([q_w.expand(self.nq, -1), k_w.expand(self.nkv, -1)])
            qkv_raw = torch.cat(
                [ops.rms_norm_ref(rows[:, :nqk], w, cfg.layer_norm_epsilon),
                 rows[:, nqk:]], dim=1).view(qkv_raw.shape)
        if not isinstance(k_cache, ops.Fp8KVCache):
            return bf16_form(qkv_raw, bias, k_cache, v_cache, *tail)
        if ops.fp8_kv_enabled():
            # the same epilogue, quantizing the K and V head rows
            return fp8_form(
                qkv_raw, bias, k_cache.codes, k_cache.scale,
                v_cache.codes, v_cache.scale, *tail)
        # REALHF_AMD_NO_FP8_KV=1, the A/B baseline and test oracle: the
        # unchanged bf16 epilogue writes into scratch caches and the rows it
        # wrote go through the reference quantizer, so the fp8 cache
        # receives the rows the kernel above would have quantized;
        # ops.attn_decode then takes the reference
        ks, vs = (torch.empty(k_cache.shape, dtype=torch.bfloat16,
                              device=qkv_raw.device) for _ in range(2))
        q = bf16_form(qkv_raw, bias, ks, vs, *tail)
        idx = (cache_seqlens.long() - 1).clamp(min=0)
        b_idx = torch.arange(ks.shape[0], device=ks.device)
        ops.fp8_kv_append_ref(ks[b_idx, idx], vs[b_idx, idx],
                              k_cache, v_cache, cache_seqlens)
        return q

    def _fused_decode(self, x, h, sp, scale, k_cache, v_cache, cache_seqlens):
        """The whole block for one decode step on HIP kernels that hand
        split-K slabs across launch boundaries: QKV slabs are summed in the
        rope/append epilogue's prologue, wo's in the fused (x + o) + mlp-norm,
        gate/up's in the activation, and the down projection folds the
        residual into its combine (_mlp_body)."""
        i = self.i
        cfg = self.cfg
        fp8 = self.fp8
        C = require_hip()
        qkv_dim = (self.nq + 2 * self.nkv) * self.hd
        merged = _maybe_merged(self.p, self._qkv_names, qkv_dim)
        if merged is not None:
            # the torch QK norm of REALHF_AMD_NO_QK_NORM_OPS=1 needs summed rows
            qkv_raw, _ = _decode_linear(
                h, merged, fp8.get("qkv"),
                slabs=not cfg.qk_rmsnorm or ops.qk_norm_ops_enabled())
        else:
            qkv_raw = torch.cat(
                [_linear(h, self.p[n]) for n in self._qkv_names], dim=-1)
        bias = None
        if f"{i}.attn.wq.bias" in self.p:
            bias = torch.cat([self.p[f"{i}.attn.w{c}.bias"] for c in "qkv"],
                             dim=0).to(qkv_raw.dtype)
        q = self._rope_append(C, qkv_raw, bias, k_cache, v_cache,
                              cache_seqlens)
        attn_out = ops.attn_decode(q, k_cache, v_cache, cache_seqlens,
                                   scale, window=self.window,
                                   softcap=self.softcap)
        attn_out = attn_out.reshape(attn_out.shape[0], self.nq * self.hd)
        # fused (x + o) + mlp-norm: plain RMS, or gemma's 1 + w mode
        add_norm = None
        if self.moe is None and cfg.norm_type == "rms":
            add_norm = C.add_rmsnorm_fwd
        elif (self.moe is None and cfg.norm_type == "gemma_rms"
              and ops.gemma_ops_enabled()):
            add_norm = C.gemma_add_rmsnorm_fwd
        wo_bias = self.p.get(f"{i}.attn.wo.bias")
        o, kind = _decode_linear(
            attn_out, self.p[f"{i}.attn.wo.weight"], fp8.get("wo"),
            slabs=(self.tp_size == 1 and wo_bias is None
                   and add_norm is not None and not cfg.post_norms))
        if kind != "slabs":
            o = mappings.reduce_from_tp_region(o)
            if wo_bias is not None:
                o = o + wo_bias
        if cfg.post_norms:
            # gemma-2 sandwich norms: wo through the combine form (the post
            # norm needs the summed rows), norm, then the usual fused
            # (x + o) + mlp-norm
            o = _norm(cfg, o, self.p[f"{i}.attn.post_ln.weight"], None)
        if add_norm is None:
            return self._mlp(x + o, sp, fp8=fp8)
        h2, x2 = add_norm(o, x, self.p[f"{i}.mlp.ln.weight"],
                          cfg.layer_norm_epsilon)
        if cfg.post_norms:
            # down without the residual fold: its output is normed first
            d = self._mlp_body(h2, sp, fp8=fp8)
            return x2 + _norm(cfg, d, self.p[f"{i}.mlp.post_ln.weight"], None)
        return self._mlp_body(h2, sp, residual=x2, fp8=fp8)

    def _mlp(self, x, sp, fp8=None):
        i = self.i
        h = _norm(self.cfg, x, self.p[f"{i}.mlp.ln.weight"], self.p.get(f"{i}.mlp.ln.bias"))
        if self.moe is not None:
            d = self.moe(h)
        else:
            d = self._mlp_body(h, sp, fp8=fp8)  # residual not folded here
        if self.cfg.post_norms:
            d = _norm(self.cfg, d, self.p[f"{i}.mlp.post_ln.weight"], None)
        return x + d

    def _mlp_body(self, h, sp, residual=None, fp8=None):
        """norm-output -> MLP delta; with `residual` (the fused decode block)
        the return value is the full residual-stream output, the residual
        added by the down projection's combine kernel where tp == 1 and
        that kernel applies.  fp8: the decode step's (q, scale) pairs for
        "gu" and "down" (FP8 weight-only decode)."""
        cfg = self.cfg
        i = self.i
        fp8 = fp8 or {}
        gated = cfg.activation in ("silu", "geglu")
        merged = None
        if gated:
            idim_local = self.p[f"{i}.mlp.gate.weight"].shape[0]
            merged = _maybe_merged(self.p, self._gu_names, 2 * idim_local)
        # fused column linear (async bwd comm) over the merged gate/up; a
        # single-up MLP keeps the mapping route
        fused_col = (self.tp_size > 1 and torch.is_grad_enabled()
                     and merged is not None)
        if not fused_col:
            h = (mappings.gather_from_sp_region(h) if sp
                 else mappings.copy_to_tp_region(h))
        if gated:
            silu = cfg.activation == "silu"  # else geglu (gemma)
            kind = "plain"
            if fused_col:
                gu = mappings.column_parallel_linear(h, merged, sp)
            elif merged is not None:
                # launch-boundary reduce: slabs summed in swiglu/geglu
                gu, kind = _decode_linear(
                    h, merged, fp8.get("gu"),
                    slabs=(self.tp_size == 1
                           and (silu or ops.gemma_ops_enabled())))
            else:
                gu = torch.cat(
                    [_linear(h, self.p[n]) for n in self._gu_names], dim=-1)
            if kind == "slabs":
                C = require_hip()
                act = (C.swiglu_fwd if silu else C.geglu_fwd)(gu)
            else:
                act = ops.swiglu(gu) if silu else ops.geglu(gu)
        else:
            up = _linear(h, self.p[f"{i}.mlp.up.weight"], self.p.get(f"{i}.mlp.up.bias"))
            act = F.gelu(up, approximate="tanh")
        down, kind = _decode_linear(
            act, self.p[f"{i}.mlp.down.weight"], fp8.get("down"),
            residual=residual if self.tp_size == 1 else None)
        if kind == "folded":
            return down  # residual already added
        down = (mappings.reduce_scatter_to_sp_region(down) if sp
                else mappings.reduce_from_tp_region(down))
        if f"{i}.mlp.down.bias" in self.p:
            down = down + self.p[f"{i}.mlp.down.bias"]
        if residual is not None:
            return residual + down
        return down


class OutputHead(nn.Module):
    """Final norm + LM head (vocab-parallel) or critic head (replicated
    1-dim output) (reference: real_llm_base.py:346-392)."""

    def __init__(self, cfg: ReaLModelConfig, params: Dict[str, torch.Tensor],
                 tied_embedding_weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.cfg = cfg
        self.p = params
        self.tied_w = tied_embedding_weight
        self.i = cfg.n_layers + 1

    def forward(self, x):
        cfg = self.cfg
        h = _norm(cfg, x, self.p[f"{self.i}.ln_f.weight"], self.p.get(f"{self.i}.ln_f.bias"))
        sp = constants.has_current() and constants.sequence_parallel()
        w = self.tied_w if self.tied_w is not None else self.p.get(f"{self.i}.head.weight")
        tp = constants.tp_world_size() if constants.has_current() else 1
        if not cfg.is_critic and tp > 1 and torch.is_grad_enabled():
            # fused (copy-to-TP | SP-gather) + GEMM on the PRE-mapping h: bwd
            # all-reduce (SP: reduce-scatter) overlaps dW.  Under SP an
            # explicit gather in front of the copy-to-TP form would sum the
            # input grad over tp twice: all-reduce, then reduce-scatter
            return self._cap(mappings.column_parallel_linear(h, w, sp))
        if sp:
            h = mappings.gather_from_sp_region(h)
        if cfg.is_critic:
            return _linear(h.float(), w.float())  # [total, 1] fp32
        h = mappings.copy_to_tp_region(h)
        if not torch.is_grad_enabled():
            # decode: the vocab head streams 262 MB of weights per token —
            # the weight-streaming skinny kernel beats hipBLASLt at M<=16
            o = ops.maybe_skinny_linear(h, w)
            if o is not None:
                return self._cap(o)
        return self._cap(_linear(h, w))  # [total, vocab/tp] — vocab-parallel logits

    def _cap(self, logits):
        """Final logit soft-cap (gemma-2), cap * tanh(logits / cap) in the
        logits' dtype; elementwise, so vocab-parallel shards take it as is."""
        cap = self.cfg.final_logit_softcap
        if not cap:
            return logits
        return torch.tanh(logits / cap) * cap
