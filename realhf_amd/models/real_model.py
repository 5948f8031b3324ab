"""ReaLModel — the flat-parameter packed-sequence transformer.

Reference semantics: realhf/impl/model/nn/real_llm_api.py (ReaLModel:82,
instantiate:183, forward:384, state_dict remap:511, async_offload:274).

All parameters of this shard (its TP shard of its PP stage's layers) live
in ONE contiguous buffer (`flat_param`); layer modules hold views.  This
is the contract that makes ZeRO-1 sharding, offload, and parameter
reallocation interval math over a single tensor (SURVEY.md §2.1
"Flat-param spec").
"""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from realhf_amd.api.model import ReaLModelConfig
from realhf_amd.base import constants, logging
from realhf_amd.models import param_layout as PL
from realhf_amd.models.layers import OutputHead, ReaLModelBlock, VocabEmbedding
from realhf_amd.utils.functional import compute_varlen_position_indices

logger = logging.getLogger("model")


class ReaLModel(nn.Module):
    def __init__(
        self,
        config: ReaLModelConfig,
        device=None,
        dtype: Optional[torch.dtype] = None,
        tp_rank: int = 0,
        tp_size: int = 1,
        pp_rank: int = 0,
        pp_size: int = 1,
        ep_rank: int = 0,
        ep_size: int = 1,
        instantiate: bool = True,
    ):
        super().__init__()
        self.config = config
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.dtype = dtype or config.torch_dtype
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.pp_rank, self.pp_size = pp_rank, pp_size
        self.ep_rank, self.ep_size = ep_rank, ep_size
        self.pipeline_partition = PL.partition_pipeline_layers(config, pp_size)
        lo, hi = self.pipeline_partition[pp_rank]
        self.layer_indices = list(range(lo, hi))
        self.layout = PL.build_flat_layout(
            config, self.layer_indices, tp_rank, tp_size,
            ep_rank=ep_rank, ep_size=ep_size,
        )

        self.flat_param: Optional[torch.Tensor] = None
        self.flat_grad: Optional[torch.Tensor] = None
        self._params: Dict[str, torch.Tensor] = {}
        self.layers = nn.ModuleList()
        self._offload_buf: Optional[torch.Tensor] = None
        self._offloaded = False
        if instantiate:
            self.instantiate()

    # ------------------------------------------------------------------
    @property
    def is_first_stage(self):
        return self.pp_rank == 0

    @property
    def is_last_stage(self):
        return self.pp_rank == self.pp_size - 1

    @property
    def num_layers_total(self):
        return self.config.n_layers + 2

    def instantiate(self):
        # zeros, not empty: the layout's 64-element alignment gaps are
        # never written by loads/inits, and garbage there makes whole-
        # buffer checksums/comparisons (bench DP check, realloc tests,
        # determinism tests) allocator-history-dependent
        self.flat_param = torch.zeros(
            self.layout.total_numel, dtype=self.dtype, device=self.device
        )
        self._map_params()
        self._build_modules()

    def _map_params(self):
        self._params = {}
        for k in self.layout.keys:
            s = self.layout.specs[k]
            self._params[k] = self.flat_param[s.start : s.end].view(s.shape)

    def _build_modules(self):
        cfg = self.config
        self.layers = nn.ModuleList()
        for idx in self.layer_indices:
            if idx == 0:
                self.layers.append(VocabEmbedding(cfg, self._params))
            elif idx == cfg.n_layers + 1:
                tied_w = None
                if cfg.tied_embedding and not cfg.is_critic:
                    assert "0.wte.weight" in self._params or self.pp_size > 1, (
                        "tied embedding with pp>1 needs the embedding group sync"
                    )
                    tied_w = self._params.get("0.wte.weight")
                self.layers.append(OutputHead(cfg, self._params, tied_w))
            else:
                self.layers.append(
                    ReaLModelBlock(cfg, idx, self._params, self.tp_size,
                                   ep_rank=self.ep_rank, ep_size=self.ep_size)
                )

    # ------------------------------------------------------------------
    @torch.no_grad()
    def random_init(self, std: float = 0.02):
        """Random init (bench path: no network, random weights)."""
        for k, t in self._params.items():
            if t.ndim >= 2:
                t.normal_(0.0, std)
            else:
                if k.endswith("ln.weight") or k.endswith("ln_f.weight"):
                    t.fill_(1.0)
                else:
                    t.zero_()

    # ------------------------------------------------------------------ LoRA
    # Reference: the "lora" ModelWrapperAbstraction (api/quickstart/
    # model.py:56 LoRAConfig, :204 wrapper with lora_keys_to_replace
    # ["c_attn.linear", "c_proj."] and the "squash" op).  Flat-param
    # design: A/B adapters live in their OWN small contiguous buffer
    # (`lora_flat`), so the LoRA optimizer is the same ZeRO-1 machinery
    # pointed at that buffer while the base flat_param stays frozen.
    def attach_lora(
        self,
        dim: int = 32,
        scaling: float = 32.0,
        keys=("attn.wq", "attn.wk", "attn.wv", "attn.wo"),
    ):
        assert getattr(self, "lora_flat", None) is None, "LoRA already attached"
        cfg = self.config
        specs: Dict[str, tuple] = {}  # name -> (start, end, shape)
        off = 0

        def _add(name, shape):
            nonlocal off
            n = shape[0] * shape[1]
            specs[name] = (off, off + n, shape)
            off += n

        for idx in self.layer_indices:
            if idx == 0 or idx == cfg.n_layers + 1:
                continue
            for k in keys:
                wname = f"{idx}.{k}.weight"
                if wname in self._params:
                    out_d, in_d = self._params[wname].shape
                    _add(f"{wname}.lora_A", (dim, in_d))
                    _add(f"{wname}.lora_B", (out_d, dim))
        self.lora_specs = specs
        self.lora_dim = dim
        self.lora_scale = scaling / dim
        self.lora_flat = torch.zeros(off, dtype=self.dtype, device=self.device)
        self.lora_grad: Optional[torch.Tensor] = None
        self._map_lora()
        with torch.no_grad():
            for name, t in self.lora_params.items():
                if name.endswith("lora_A"):
                    # deterministic per-name seed: identical on every rank
                    # (replicated-A TP shards must match across tp ranks).
                    # NOTE zlib.crc32, not hash() — python str hashes are
                    # salted per process.
                    import zlib

                    g = torch.Generator(device=t.device)
                    g.manual_seed(zlib.crc32(name.encode()) % (2**31))
                    t.normal_(0.0, 1.0 / dim, generator=g)
        self._inject_lora()

    def _map_lora(self):
        self.lora_params: Dict[str, torch.Tensor] = {}
        for name, (s, e, shape) in self.lora_specs.items():
            self.lora_params[name] = self.lora_flat[s:e].view(shape)

    def _inject_lora(self):
        for blk in self.layers:
            if not isinstance(blk, ReaLModelBlock):
                continue
            i = blk.i
            d = {}
            for short in ("wq", "wk", "wv", "wo"):
                a = self.lora_params.get(f"{i}.attn.{short}.weight.lora_A")
                b = self.lora_params.get(f"{i}.attn.{short}.weight.lora_B")
                if a is not None:
                    d[short] = (a, b)
            blk.lora = d
            blk.lora_scale = self.lora_scale

    def lora_grad_view(self, name: str) -> torch.Tensor:
        s, e, shape = self.lora_specs[name]
        return self.lora_grad[s:e].view(shape)

    @torch.no_grad()
    def squash_lora(self):
        """Merge the adapters into the base weights and detach LoRA
        (reference: lora_op_after_creation="squash")."""
        for wname in {n.rsplit(".lora_", 1)[0] for n in self.lora_specs}:
            a = self.lora_params[f"{wname}.lora_A"].float()
            b = self.lora_params[f"{wname}.lora_B"].float()
            w = self._params[wname]
            w.add_((b @ a).to(w.dtype) * self.lora_scale)
        self.lora_flat = None
        self.lora_specs = {}
        self.lora_params = {}
        for blk in self.layers:
            if isinstance(blk, ReaLModelBlock):
                blk.lora = {}

    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.clone() for k, v in self.lora_params.items()}

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]):
        with torch.no_grad():
            for k, v in sd.items():
                self.lora_params[k].copy_(v)

    # ------------------------------------------------------------------ fwd
    def forward(
        self,
        packed_input_ids: Optional[torch.Tensor] = None,
        cu_seqlens: Optional[torch.Tensor] = None,
        max_seqlen: Optional[int] = None,
        hidden_states: Optional[torch.Tensor] = None,
        positions: Optional[torch.Tensor] = None,
        kv_caches: Optional[List[torch.Tensor]] = None,  # [(k,v)] per local block
        cache_seqlens: Optional[torch.Tensor] = None,
        decode: bool = False,
        logprob_labels: Optional[torch.Tensor] = None,
        logprob_inv_temperature: float = 1.0,
    ):
        """Run this PP stage.  First stage consumes packed_input_ids, later
        stages consume hidden_states.  Returns hidden states (mid stages)
        or logits/values (last stage).  With logprob_labels [total] the last
        stage returns fp32 [total] log-probs of those labels instead of
        logits (OutputHead.logprobs; inference only)."""
        assert self._offloaded is False, "model is offloaded; reload first"
        cfg = self.config
        if decode:
            assert cache_seqlens is not None
            positions = cache_seqlens.long() - 1
            cu = None
            mx = None
        else:
            total = (
                packed_input_ids.shape[0]
                if packed_input_ids is not None
                else hidden_states.shape[0]
            )
            if positions is None:
                positions = compute_varlen_position_indices(total, cu_seqlens)
            cu = cu_seqlens
            mx = max_seqlen

        x = hidden_states
        cache_i = 0
        use_ckpt = (
            constants.has_current()
            and constants.gradient_checkpointing()
            and torch.is_grad_enabled()
            and not decode
        )
        for idx, layer in zip(self.layer_indices, self.layers):
            if idx == 0:
                x = layer(packed_input_ids, positions)
            elif idx == cfg.n_layers + 1:
                if logprob_labels is not None:
                    x = layer.logprobs(x, logprob_labels, logprob_inv_temperature)
                else:
                    x = layer(x)
            else:
                kc = vc = None
                if kv_caches is not None:
                    kc, vc = kv_caches[cache_i]
                    cache_i += 1
                if use_ckpt:
                    x = torch.utils.checkpoint.checkpoint(
                        layer, x, cu, mx, positions, kc, vc, cache_seqlens, decode,
                        use_reentrant=False,
                    )
                else:
                    x = layer(
                        x, cu, mx, positions,
                        k_cache=kc, v_cache=vc,
                        cache_seqlens=cache_seqlens, decode=decode,
                    )
        return x

    # ---------------------------------------------------------- state dict
    def state_dict(self, *args, **kwargs):  # noqa: D102 — canonical keys
        return {k: v for k, v in self._params.items()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        with torch.no_grad():
            for k, v in self._params.items():
                if k in sd:
                    v.copy_(sd[k].to(v.dtype))
                elif strict:
                    raise KeyError(k)
        return self

    def named_parameters(self, *a, **kw):
        for k, v in self._params.items():
            yield k, v

    @property
    def n_local_params(self):
        return self.layout.total_numel

    # ------------------------------------------------------------- offload
    def _side_stream(self):
        if not hasattr(self, "_offload_stream"):
            self._offload_stream = torch.cuda.Stream()
        return self._offload_stream

    def async_offload(self, non_blocking: bool = True):
        """Copy flat params to pinned host memory and free the device
        buffer (reference: real_llm_api.py:274).  Used for non-trainable
        roles between their MFCs.  With non_blocking=True the D2H runs on
        a side stream overlapped with subsequent compute; the allocator
        defers block reuse via record_stream."""
        if self._offloaded:
            return
        if self._offload_buf is None:
            self._offload_buf = torch.empty(
                self.flat_param.shape, dtype=self.dtype, device="cpu",
                pin_memory=torch.cuda.is_available(),
            )
        if non_blocking and self.flat_param.is_cuda:
            s = self._side_stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._offload_buf.copy_(self.flat_param, non_blocking=True)
            self.flat_param.record_stream(s)
        else:
            self._offload_buf.copy_(self.flat_param, non_blocking=False)
        self.flat_param = None
        self._params = {}
        self.layers = nn.ModuleList()
        self._offloaded = True

    # ---------------------------------------------- dp-shard (ZeRO-3 style)
    def shard_to_dp(self, group=None):
        """ZeRO-3-style release for FROZEN roles: keep only this rank's
        1/dp slice of the flat buffer; peers hold the rest.  Resident
        memory drops to shard size between MFCs, and `gather_from_dp`
        restores the full buffer with ONE RCCL all-gather over xGMI
        (~0.8 s for 70B at 8 ranks vs ~2.2 s for a PCIe host reload —
        the 288 GB/xGMI-native alternative to `async_offload`).
        Reference counterpart: DeepSpeed ZeRO-3 param sharding
        (deepspeed.py:276-359), which the reference cannot combine with
        realloc; here the shard is just a view of the flat layout."""
        import torch.distributed as dist

        if self._offloaded or getattr(self, "_dp_sharded", False):
            return
        g = constants.grid() if constants.has_current() else None
        group = group or (g.dp_group() if g is not None else None)
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        if world == 1:
            return
        n = self.flat_param.numel()
        pad = (-n) % world
        self._dp_shard_meta = (n, pad, group)
        padded = self.flat_param
        if pad:
            padded = torch.cat([self.flat_param,
                                self.flat_param.new_zeros(pad)])
        rank = dist.get_rank(group)
        l = (n + pad) // world
        self._dp_shard = padded[rank * l:(rank + 1) * l].clone()
        self.flat_param = None
        self._params = {}
        self.layers = nn.ModuleList()
        self._dp_sharded = True

    def gather_from_dp(self):
        """Restore the full flat buffer from the DP shards (one
        all-gather) and rebuild the module views."""
        import torch.distributed as dist

        if not getattr(self, "_dp_sharded", False):
            return
        n, pad, group = self._dp_shard_meta
        full = torch.empty(n + pad, dtype=self._dp_shard.dtype,
                           device=self._dp_shard.device)
        try:
            backend = dist.get_backend(group)
        except Exception:
            backend = "nccl"
        if backend == "gloo" and self._dp_shard.is_cuda:
            # gloo lacks CUDA all-gather (1-GPU multi-rank tests): one
            # broadcast per shard; RCCL takes the single-collective path
            world = dist.get_world_size(group)
            ranks = (dist.get_process_group_ranks(group)
                     if group is not None else list(range(world)))
            l = (n + pad) // world
            me = dist.get_rank(group)
            for r in range(world):
                piece = full[r * l:(r + 1) * l]
                if r == me:
                    piece.copy_(self._dp_shard)
                dist.broadcast(piece, src=ranks[r], group=group)
        else:
            dist.all_gather_into_tensor(full, self._dp_shard.contiguous(),
                                        group=group)
        self.flat_param = full[:n]
        self._dp_shard = None
        self._dp_sharded = False
        self._map_params()
        self._build_modules()

    def start_reload(self):
        """Kick the H2D reload on the side stream (overlaps with whatever
        compute is running); finish_reload() must be called before use."""
        if not self._offloaded or getattr(self, "_reload_pending", None):
            return
        if not torch.cuda.is_available() or not self.device.type == "cuda":
            return
        s = self._side_stream()
        with torch.cuda.stream(s):
            flat = torch.empty(
                self._offload_buf.shape, dtype=self.dtype, device=self.device
            )
            flat.copy_(self._offload_buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
        self._reload_pending = (flat, ev)

    def reload_from_offload(self):
        if not self._offloaded:
            return
        pending = getattr(self, "_reload_pending", None)
        if pending is not None:
            flat, ev = pending
            torch.cuda.current_stream().wait_event(ev)
            flat.record_stream(torch.cuda.current_stream())
            self.flat_param = flat
            self._reload_pending = None
        else:
            self.flat_param = self._offload_buf.to(self.device, non_blocking=False)
        self._map_params()
        self._build_modules()
        self._offloaded = False

    # -------------------------------------------------------------- resize
    def allocate_grad_buffer(self):
        if self.flat_grad is None or self.flat_grad.numel() != self.flat_param.numel():
            self.flat_grad = torch.zeros_like(self.flat_param)
        return self.flat_grad

    def grad_view(self, key: str) -> torch.Tensor:
        s = self.layout.specs[key]
        return self.flat_grad[s.start : s.end].view(s.shape)

    def param_view(self, key: str) -> torch.Tensor:
        return self._params[key]


# ---------------------------------------------------------------------------
def make_real_model(
    config: ReaLModelConfig,
    model_name: Optional[str] = None,
    device=None,
    dtype=None,
) -> ReaLModel:
    """Factory reading TP/PP geometry from the registered grid (when a
    model scope/grid exists) or building a single-shard model."""
    if model_name is not None and constants.has_model(model_name):
        g = constants.grid_of(model_name)
        return ReaLModel(
            config, device=device, dtype=dtype,
            tp_rank=g.tp_rank, tp_size=g.tp_size,
            pp_rank=g.pp_rank, pp_size=g.pp_size,
        )
    return ReaLModel(config, device=device, dtype=dtype)
