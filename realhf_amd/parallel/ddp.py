"""Native ZeRO-1 distributed optimizer on the flat parameter buffer.

Replaces the reference's Megatron-core DDP + DistributedOptimizer
(realhf/impl/model/backend/megatron.py:822-1007) with a design that owns
the flat layout end-to-end, so realloc compatibility is by construction
(SURVEY.md §7 stage 5 rationale).

Mechanics (per train step, DP size d):
  1. backward accumulates into the padded flat grad buffer (param.grad
     views);
  2. one reduce-scatter of the flat grad over DP; global grad-norm clip
     (DP-reduced).  With REALHF_AMD_ZERO_OVERLAP=1 the reduce-scatter
     runs per BUCKET as the backward completes each bucket's grads
     (per-bucket ownership; see the overlap block in __init__).
  3. fused AdamW (HIP kernel) updates the fp32 master shard of this rank
     and writes bf16 back into the param shard;
  4. all-gather of param shards into the flat param buffer (one RCCL
     all-gather over xGMI; 288 GB HBM argues for few, large collectives).

With dp == 1 every collective is skipped and this is a fused-AdamW
mixed-precision optimizer.
"""
import dataclasses
import math
import os
from typing import Dict, List

import torch
import torch.distributed as dist

from realhf_amd.base import constants, logging
from realhf_amd.ops import functional as ops

logger = logging.getLogger("ddp")


@dataclasses.dataclass
class OptimizerConfig:
    type: str = "adam"
    lr: float = 1e-5
    weight_decay: float = 0.05
    beta1: float = 0.9
    beta2: float = 0.95
    eps: float = 1e-5
    min_lr_ratio: float = 0.0
    lr_scheduler_type: str = "cosine"  # cosine | linear | constant
    warmup_steps_proportion: float = 0.02
    gradient_clipping: float = 1.0
    offload: bool = False  # optimizer states in host memory (70B tier)
    # 1 = ZeRO-1 (shard optimizer states); 2 = ZeRO-2 (additionally never
    # hold a full-model grad buffer: per-microbatch bucket staging +
    # reduce-scatter accumulation into the shard).  Reference counterpart:
    # DeepSpeed zero_stage (deepspeed.py:276-359).
    zero_stage: int = 1


class LoRAFacade:
    """Adapter that lets ZeRO1Optimizer drive a ReaLModel's LoRA buffer:
    exposes flat_param/flat_grad/_params/grad_view backed by the model's
    lora_* attributes, so adapters get the same sharded AdamW + LR
    schedule + clipping while the base flat_param stays frozen."""

    def __init__(self, model):
        self._m = model
        assert getattr(model, "lora_flat", None) is not None, "attach_lora first"
        self.flat_param = model.lora_flat
        self.flat_grad = None

    def _map_params(self):
        self._m.lora_flat = self.flat_param
        self._m._map_lora()
        self._m._inject_lora()

    def _build_modules(self):
        pass

    @property
    def _params(self):
        return self._m.lora_params

    def grad_view(self, k):
        self._m.lora_grad = self.flat_grad
        return self._m.lora_grad_view(k)


class ZeRO1Optimizer:
    def __init__(
        self,
        model,  # ReaLModel
        cfg: OptimizerConfig,
        total_train_steps: int = 1000,
        bucket_size: int = 40_000_000,  # 40M elements ≈ 80 MB bf16 buckets
    ):
        self.model = model
        self.cfg = cfg
        self.total_steps = max(1, total_train_steps)
        self.warmup_steps = int(cfg.warmup_steps_proportion * self.total_steps)
        self.step_count = 0

        g = constants.grid() if constants.has_current() else None
        self.dp_group = g.dp_group() if g is not None else None
        self.dp_size = g.dp_size if g is not None else 1
        self.dp_rank = g.dp_rank if g is not None else 0
        # REPLICATED params (layernorms, critic head) exist identically
        # on every tp rank.  Two uses: (a) under SP their grads are
        # per-tp-rank partials and must sum over tp BEFORE the DP
        # reduce-scatter; (b) the global grad norm must count them ONCE,
        # not tp x (they are discounted by 1/tp before the model-group
        # norm reduction below).
        self._repl_ivs = []  # flat intervals of replicated params
        # the intervals step() sums over tp, each exactly once: under SP all
        # of _repl_ivs; without SP only those whose grads are partial sums
        # over a rank's heads (PL.grad_is_head_partial: qwen3's q/k norms)
        self._sp_repl_ivs = []
        self.tp_group = None
        self.tp_size = g.tp_size if g is not None else 1
        self.pp_size = g.pp_size if g is not None else 1
        self.model_group = g.model_group() if g is not None else None
        if (g is not None and g.tp_size > 1 and hasattr(model, "layout")):
            from realhf_amd.models import param_layout as PL

            self.tp_group = g.tp_group()
            for k in model.layout.keys:
                kind = PL.key_kind(k)
                if kind == "head":
                    kind = (PL.REPLICATED if model.config.is_critic
                            else PL.VOCAB)
                if kind == PL.REPLICATED:
                    sp_ = model.layout.specs[k]
                    self._repl_ivs.append((sp_.start, sp_.end))
                    if PL.grad_is_head_partial(k):
                        self._sp_repl_ivs.append((sp_.start, sp_.end))
            if constants.has_current() and constants.sequence_parallel():
                self._sp_repl_ivs = list(self._repl_ivs)

        n = model.flat_param.numel()
        # pad so every DP shard is 256-element aligned
        self.pad = (-n) % (256 * self.dp_size)
        self.n_pad = n + self.pad
        self.shard_size = self.n_pad // self.dp_size
        dev = model.flat_param.device

        # padded param buffer: re-point the model's flat buffer into it
        if self.pad > 0 or True:
            new_param = torch.zeros(self.n_pad, dtype=model.flat_param.dtype, device=dev)
            new_param[:n].copy_(model.flat_param)
            model.flat_param = new_param[:n]
            self._param_padded = new_param
            model._map_params()
            model._build_modules()

        # ---- ZeRO-2: no full-model grad buffer ever exists -------------
        # Autograd allocates each param's grad; a post-accumulate hook
        # stages it into a pooled bucket buffer and frees it.  Complete
        # buckets reduce-scatter immediately and ACCUMULATE into
        # grad_shard (one RS per bucket per microbatch — the classic
        # ZeRO-2 comm/memory trade).  Peak grad memory = a few buckets
        # instead of a full model copy.
        self.zero2 = (
            cfg.zero_stage >= 2
            and self.dp_size > 1
            and self.tp_size == 1   # SP tp-reduce needs full-grad intervals
            and hasattr(model, "layout")
        )
        if cfg.zero_stage >= 2 and not self.zero2:
            logger.warning(
                "zero_stage=2 requested but unsupported here "
                "(needs dp>1, tp==1); falling back to ZeRO-1")
        if self.zero2:
            self.grad_padded = None
            model.flat_grad = None
        else:
            self.grad_padded = torch.zeros(
                self.n_pad, dtype=model.flat_param.dtype, device=dev)
            model.flat_grad = self.grad_padded[:n]

        s0 = self.dp_rank * self.shard_size
        s1 = s0 + self.shard_size
        self.shard_bounds = (s0, s1)
        state_dev = "cpu" if cfg.offload else dev

        # ---- bucketed comm/compute overlap (opt-in, dp>1) --------------
        # With REALHF_AMD_ZERO_OVERLAP=1, grads reduce-scatter per BUCKET
        # as soon as the backward has produced every grad overlapping the
        # bucket (post-accumulate-grad hooks, armed for the LAST
        # minibatch only).  Ownership becomes per-bucket (rank r owns
        # slice r of each bucket) so RS outputs land contiguously in
        # grad_shard; master/exp_avg use the same per-bucket layout and
        # params all-gather back per bucket.
        self.bucket_size = bucket_size
        # DEFAULT ON since round 2 (REALHF_AMD_ZERO_OVERLAP=0 opts out):
        # the dp>1 CPU multiprocess tests run this path on every PR, and
        # it is the configuration the 8-GPU scale bench runs with.
        self.overlap_comm = (
            os.environ.get("REALHF_AMD_ZERO_OVERLAP", "1") != "0"
            and self.dp_size > 1
            and hasattr(model, "layout")
            and self.tp_size == 1  # tp: SP tp-reduce + norm discount
                                   # need the contiguous shard layout
            and not self.zero2     # ZeRO-2 has its own per-mb staging
        )
        if self.overlap_comm and self._gloo_cuda():
            self.overlap_comm = False  # async RS unavailable on gloo+CUDA
        if self.overlap_comm or self.zero2:
            align = 256 * self.dp_size
            self._bsz = max(align, (bucket_size // align) * align)
            self.buckets = []  # (b0, b1, shard_off)
            off, soff = 0, 0
            while off < self.n_pad:
                b1 = min(self.n_pad, off + self._bsz)
                self.buckets.append((off, b1, soff))
                soff += (b1 - off) // self.dp_size
                off = b1
            pieces = []
            for b0, b1, _ in self.buckets:
                l = (b1 - b0) // self.dp_size
                pieces.append(
                    self._param_padded[b0 + self.dp_rank * l:
                                       b0 + (self.dp_rank + 1) * l])
            self.master = torch.cat(pieces).to(torch.float32).to(state_dev)
            self._shard_bf16 = torch.empty(
                self.shard_size, dtype=model.flat_param.dtype, device=dev)
            # param -> overlapped bucket ids
            self._param_buckets = {}
            for k in model.layout.keys:
                sp = model.layout.specs[k]
                self._param_buckets[k] = list(
                    range(sp.start // self._bsz, (sp.end - 1) // self._bsz + 1))
            self._bucket_left: List[int] = []
            # safe default: an engine that never arms (or a backward that
            # skipped arming) flushes every bucket synchronously at step()
            self._reduced: List[bool] = [False] * len(self.buckets)
            self._works: list = []
            self._armed = False
            if self.zero2:
                self._z2_pool: List[torch.Tensor] = []     # [bsz] staging
                self._z2_scratch: List[torch.Tensor] = []  # [bsz/dp] RS out
                self._z2_active: Dict[int, torch.Tensor] = {}
                self._z2_left = None   # per-microbatch outstanding counts
                self._z2_inflight: list = []  # (work, buf, scr, soff, l)
                self._z2_max_inflight = int(
                    os.environ.get("REALHF_AMD_Z2_INFLIGHT", 4))
        elif cfg.offload:
            # chunked fp32 conversion: a whole-shard .float() on device
            # would spike 2x shard bytes (275 GB for 70B at dp1)
            self.master = torch.empty(self.shard_size, dtype=torch.float32,
                                      device="cpu")
            ch = 64 * 1024 * 1024
            for c0 in range(0, self.shard_size, ch):
                c1 = min(self.shard_size, c0 + ch)
                self.master[c0:c1].copy_(
                    self._param_padded[s0 + c0:s0 + c1].float())
        else:
            self.master = self._param_padded[s0:s1].to(torch.float32).to(state_dev)
        if cfg.offload and dev.type == "cuda":
            # pinned host states: the offloaded step streams chunks
            # through the GPU (H2D -> fused AdamW -> D2H) on a side
            # stream, double-buffered — PCIe-bound instead of CPU-bound
            # (reference counterpart: DeepSpeed ZeRO-offload,
            # deepspeed.py:276-359; round-1 blocked on a sync .cpu()).
            try:
                self.master = self.master.pin_memory()
            except RuntimeError:
                logger.warning("pin_memory failed; offload uses pageable host mem")
        self.exp_avg = torch.zeros_like(self.master)
        self.exp_avg_sq = torch.zeros_like(self.master)
        if cfg.offload and dev.type == "cuda" and self.master.is_pinned():
            try:
                self.exp_avg = self.exp_avg.pin_memory()
                self.exp_avg_sq = self.exp_avg_sq.pin_memory()
            except RuntimeError:
                pass
        self.grad_shard = torch.empty(
            self.shard_size, dtype=model.flat_param.dtype, device=dev
        )
        if cfg.offload and dev.type == "cuda":
            self._off_chunk = int(os.environ.get(
                "REALHF_AMD_OFFLOAD_CHUNK", 32 * 1024 * 1024
            ))  # fp32 elems: 128 MB/tensor default
            self._off_up_stream = torch.cuda.Stream()
            self._off_down_stream = torch.cuda.Stream()
            self._off_stage = [
                {
                    "master": torch.empty(self._off_chunk, dtype=torch.float32, device=dev),
                    "m": torch.empty(self._off_chunk, dtype=torch.float32, device=dev),
                    "v": torch.empty(self._off_chunk, dtype=torch.float32, device=dev),
                    "h2d": torch.cuda.Event(),
                    "done": torch.cuda.Event(),
                    "d2h_done": torch.cuda.Event(),
                }
                for _ in range(2)
            ]

        self._grad_views_attached = False
        # async param all-gathers left in flight by step(defer_allgather=
        # True) — waited by finish_allgather() (engines call it before
        # any param use).  Lets the LAST PPO minibatch's all-gather hide
        # under the next MFC (e.g. critic AG under the 2.7 s generation).
        self._pending_ag: List = []

    # ------------------------------------------------------------------
    def attach_grads(self):
        """Point every param's .grad at its flat-grad view so autograd
        accumulates in place.  ZeRO-2 never attaches views: autograd
        allocates each grad, the hook stages + frees it."""
        for k, p in self.model._params.items():
            if not p.requires_grad:
                p.requires_grad_(True)
            if self.zero2:
                p.register_post_accumulate_grad_hook(self._make_z2_hook(k))
                continue
            p.grad = self.model.grad_view(k)
            if self.overlap_comm:
                bids = self._param_buckets.get(k)
                if bids is not None:
                    p.register_post_accumulate_grad_hook(
                        self._make_bucket_hook(bids))
        self._grad_views_attached = True

    # ---------------- bucketed overlap machinery ----------------------
    def _make_bucket_hook(self, bids):
        def hook(_p):
            if not self._armed:
                return
            for b in bids:
                self._bucket_left[b] -= 1
                if self._bucket_left[b] == 0:
                    self._flush_bucket(b)
        return hook

    def arm_overlap(self):
        """Call right before the LAST minibatch's backward: buckets
        reduce-scatter as soon as their grads are complete."""
        if not self.overlap_comm:
            return
        counts = [0] * len(self.buckets)
        for k in self.model._params:
            for b in self._param_buckets.get(k, ()):
                counts[b] += 1
        self._bucket_left = counts
        self._reduced = [False] * len(self.buckets)
        self._works = []
        self._armed = True

    def _flush_bucket(self, b):
        b0, b1, soff = self.buckets[b]
        l = (b1 - b0) // self.dp_size
        w = dist.reduce_scatter_tensor(
            self.grad_shard[soff:soff + l], self.grad_padded[b0:b1],
            op=dist.ReduceOp.AVG, group=self.dp_group, async_op=True,
        )
        self._works.append(w)
        self._reduced[b] = True

    # ---------------- ZeRO-2 machinery --------------------------------
    def _make_z2_hook(self, key):
        sp = self.model.layout.specs[key]
        bids = self._param_buckets[key]

        def hook(p):
            g = p.grad
            if g is None:
                return
            if self._z2_left is None:
                self._z2_arm()
            flat = g.reshape(-1)
            for b in bids:
                b0, b1, _ = self.buckets[b]
                buf = self._z2_active.get(b)
                if buf is None:
                    buf = self._z2_acquire(b1 - b0)
                    self._z2_active[b] = buf
                lo, hi = max(sp.start, b0), min(sp.end, b1)
                buf[lo - b0:hi - b0].copy_(flat[lo - sp.start:hi - sp.start])
                self._z2_left[b] -= 1
                if self._z2_left[b] == 0:
                    self._z2_rs(b)
            p.grad = None  # the full grad never outlives its bucket copy

        return hook

    def _z2_arm(self):
        counts = [0] * len(self.buckets)
        for k in self.model._params:
            for b in self._param_buckets.get(k, ()):
                counts[b] += 1
        self._z2_left = counts

    def _z2_acquire(self, length):
        if not self._z2_pool and len(self._z2_inflight) >= self._z2_max_inflight:
            self._z2_harvest(1)
        full = (self._z2_pool.pop() if self._z2_pool else torch.empty(
            self._bsz, dtype=self.model.flat_param.dtype,
            device=self.model.flat_param.device))
        buf = full[:length]
        buf.zero_()  # params missing at flush time contribute zero
        return buf

    def _z2_rs(self, b):
        """Reduce-scatter one staged bucket; result accumulates into
        grad_shard at harvest time (each microbatch's loss is already
        scaled by 1/n_mbs, so summing per-mb averages is the full-batch
        average)."""
        b0, b1, soff = self.buckets[b]
        buf = self._z2_active.pop(b)
        l = (b1 - b0) // self.dp_size
        scr = (self._z2_scratch.pop() if self._z2_scratch else torch.empty(
            self._bsz // self.dp_size, dtype=buf.dtype, device=buf.device))
        if self._gloo_cuda():
            # gloo lacks CUDA reduce-scatter: all-reduce + local slice
            # (same fallback as the ZeRO-1 path; memory win void, but the
            # 2-ranks-1-GPU tests exercise identical semantics)
            w = dist.all_reduce(buf, group=self.dp_group, async_op=True)
            self._z2_inflight.append((w, buf, scr, soff, l, b))
            return
        w = dist.reduce_scatter_tensor(
            scr[:l], buf, op=dist.ReduceOp.AVG, group=self.dp_group,
            async_op=True)
        self._z2_inflight.append((w, buf, scr, soff, l, None))

    def _z2_harvest(self, k=None):
        take = len(self._z2_inflight) if k is None else min(
            k, len(self._z2_inflight))
        for w, buf, scr, soff, l, b in self._z2_inflight[:take]:
            w.wait()
            if b is not None:  # gloo-CUDA all-reduce fallback: slice + avg
                self.grad_shard[soff:soff + l] += (
                    buf[self.dp_rank * l:(self.dp_rank + 1) * l]
                    / self.dp_size)
            else:
                self.grad_shard[soff:soff + l] += scr[:l]
            self._z2_pool.append(self._z2_repool(buf))
            self._z2_scratch.append(scr)
        del self._z2_inflight[:take]

    @staticmethod
    def _z2_repool(buf):
        # recover the full pooled tensor from a length-limited view
        # (the last bucket is shorter than _bsz)
        full = torch.empty(0, dtype=buf.dtype, device=buf.device)
        full.set_(buf.untyped_storage(), 0,
                  (buf.untyped_storage().nbytes() // buf.element_size(),))
        return full

    def end_microbatch(self):
        """ZeRO-2: called by the engine after every backward — flush
        partially-filled buckets (missing slices are zero) and re-arm for
        the next microbatch.  No-op otherwise."""
        if not self.zero2 or self._z2_left is None:
            return
        for b in list(self._z2_active):
            self._z2_rs(b)
        self._z2_left = None

    def finish_allgather(self):
        for w in self._pending_ag:
            w.wait()
        self._pending_ag = []

    def zero_grad(self):
        self.finish_allgather()
        if self.zero2:
            self._z2_harvest()  # drop any stale in-flight RS results
            self._z2_left = None
            self._z2_active.clear()
            self.grad_shard.zero_()
        else:
            self.grad_padded.zero_()
        if self.overlap_comm:
            self._armed = False  # a failed backward must not leave stale state
            self._works = []
        if not self._grad_views_attached:
            self.attach_grads()

    def _gloo_cuda(self) -> bool:
        try:
            return (self.model.flat_param.is_cuda
                    and dist.get_backend(self.dp_group) == "gloo")
        except Exception:
            return False

    # ------------------------------------------------------------------
    def _lr(self) -> float:
        c = self.cfg
        s = self.step_count
        if s < self.warmup_steps:
            return c.lr * (s + 1) / max(1, self.warmup_steps)
        frac = (s - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps)
        frac = min(1.0, frac)
        lo = c.lr * c.min_lr_ratio
        if c.lr_scheduler_type == "cosine":
            return lo + 0.5 * (c.lr - lo) * (1 + math.cos(math.pi * frac))
        if c.lr_scheduler_type == "linear":
            return c.lr - (c.lr - lo) * frac
        return c.lr

    @torch.no_grad()
    def step(self, defer_allgather: bool = False) -> Dict[str, float]:
        self.step_count += 1
        cfg = self.cfg
        dev = self.model.flat_param.device

        # 0. sum over the tp group the replicated params' grads that are
        #    per-rank partials (SP: all of them; else the head-partial ones)
        if self._sp_repl_ivs:
            for a, b in self._sp_repl_ivs:
                dist.all_reduce(self.grad_padded[a:b], group=self.tp_group)

        # 1. reduce-scatter grads over DP (average)
        if self.zero2:
            # every microbatch already reduce-scattered; drain the tail
            self.end_microbatch()
            self._z2_harvest()
            gshard = self.grad_shard
        elif self.overlap_comm:
            # flush buckets the hooks missed (unused params / not armed)
            for b in range(len(self.buckets)):
                if not self._reduced[b]:
                    self._flush_bucket(b)
            for w in self._works:
                w.wait()
            self._works = []
            self._armed = False
            # ready for the next step even if the engine never re-arms
            self._reduced = [False] * len(self.buckets)
            gshard = self.grad_shard
        elif self.dp_size > 1:
            if self._gloo_cuda():
                # gloo lacks CUDA reduce-scatter: all-reduce + local slice
                dist.all_reduce(self.grad_padded, group=self.dp_group)
                self.grad_padded /= self.dp_size
                s0_, s1_ = self.shard_bounds
                self.grad_shard.copy_(self.grad_padded[s0_:s1_])
            else:
                dist.reduce_scatter_tensor(
                    self.grad_shard, self.grad_padded, op=dist.ReduceOp.AVG,
                    group=self.dp_group,
                )
            gshard = self.grad_shard
        else:
            gshard = self.grad_padded  # no copy needed at dp==1

        # 2. grad-norm clip — computed WITHOUT materializing an fp32 copy
        #    (a 7B fp32 grad copy is a 28 GiB spike).  The clip factor is
        #    folded into the AdamW kernel's grad_scale.
        grad_norm = None
        gscale = 1.0
        if cfg.gradient_clipping and cfg.gradient_clipping > 0:
            sq = torch.linalg.vector_norm(gshard, dtype=torch.float32) ** 2
            if self.tp_size > 1 and not self.overlap_comm:
                # replicated params appear on every tp rank: count once
                s0_, s1_ = self.shard_bounds
                for a, b in self._repl_ivs:
                    lo, hi = max(a, s0_), min(b, s1_)
                    if lo < hi:
                        part = torch.linalg.vector_norm(
                            gshard[lo - s0_:hi - s0_],
                            dtype=torch.float32) ** 2
                        sq -= part * (self.tp_size - 1) / self.tp_size
            if self.model_group is not None and (
                    self.dp_size > 1 or self.tp_size > 1
                    or self.pp_size > 1):
                # model-group reduction (dp x tp x pp): one global norm,
                # identical clip factor on every rank
                dist.all_reduce(sq, group=self.model_group)
            grad_norm = float(sq.sqrt())
            if not math.isfinite(grad_norm):
                logger.warning("non-finite grad norm %s — skipping step", grad_norm)
                return {"lr": self._lr(), "grad_norm": grad_norm, "skipped": 1.0}
            clip = cfg.gradient_clipping / (grad_norm + 1e-6)
            gscale = min(1.0, clip)

        # 3. AdamW on this rank's shard (bf16 grads read directly)
        lr = self._lr()
        s0, s1 = self.shard_bounds
        param_shard = (self._shard_bf16 if (self.overlap_comm or self.zero2)
                       else self._param_padded[s0:s1])
        if cfg.offload and dev.type == "cuda":
            self._adamw_offloaded(gshard, param_shard, lr, gscale)
        elif cfg.offload:
            # CPU path (tests / no GPU): states live on host, torch math
            g_in = gshard.float().cpu()
            ops.fused_adamw(
                self.master, g_in, self.exp_avg, self.exp_avg_sq,
                lr=lr, beta1=cfg.beta1, beta2=cfg.beta2, eps=cfg.eps,
                weight_decay=cfg.weight_decay, step=self.step_count,
                bf16_out=None, grad_scale=gscale,
            )
            param_shard.copy_(self.master.to(param_shard.dtype))
        else:
            ops.fused_adamw(
                self.master, gshard, self.exp_avg, self.exp_avg_sq,
                lr=lr, beta1=cfg.beta1, beta2=cfg.beta2, eps=cfg.eps,
                weight_decay=cfg.weight_decay, step=self.step_count,
                bf16_out=param_shard, grad_scale=gscale,
            )

        # 4. all-gather updated params
        if self.overlap_comm or self.zero2:
            works = []
            for b0, b1, soff in self.buckets:
                l = (b1 - b0) // self.dp_size
                works.append(dist.all_gather_into_tensor(
                    self._param_padded[b0:b1], self._shard_bf16[soff:soff + l],
                    group=self.dp_group, async_op=True))
            if defer_allgather:
                self._pending_ag = works
            else:
                for w in works:
                    w.wait()
        elif self.dp_size > 1:
            if self._gloo_cuda():
                # gloo lacks CUDA all-gather: one broadcast per dp rank
                for r in range(self.dp_size):
                    piece = self._param_padded[r * self.shard_size:
                                               (r + 1) * self.shard_size]
                    if r == self.dp_rank:
                        piece.copy_(param_shard)
                    src_g = dist.get_process_group_ranks(self.dp_group)[r] \
                        if self.dp_group is not None else r
                    dist.broadcast(piece, src=src_g, group=self.dp_group)
            else:
                w = dist.all_gather_into_tensor(
                    self._param_padded, param_shard.contiguous(),
                    group=self.dp_group, async_op=True
                )
                if defer_allgather:
                    self._pending_ag = [w]
                else:
                    w.wait()
        out = {"lr": lr}
        if grad_norm is not None:
            out["grad_norm"] = grad_norm
        return out

    @torch.no_grad()
    def _adamw_offloaded(self, gshard, param_shard, lr, gscale):
        """Pipelined offloaded AdamW: host-resident fp32 states stream
        through the GPU in double-buffered chunks.  Per chunk i:
        H2D(master,m,v) on the side stream -> fused AdamW on the default
        stream (writes the bf16 param-shard chunk in place) -> D2H of the
        updated states back to pinned host memory.  Chunk i+1's uploads
        overlap chunk i's compute+downloads, so the step runs at PCIe
        bandwidth instead of blocking on a whole-shard sync copy."""
        cfg = self.cfg
        n = self.shard_size
        cur = torch.cuda.current_stream()
        us, ds = self._off_up_stream, self._off_down_stream
        us.wait_stream(cur)  # grads must be final before chunks start
        chunks = list(range(0, n, self._off_chunk))
        for idx, c0 in enumerate(chunks):
            c1 = min(n, c0 + self._off_chunk)
            l = c1 - c0
            st = self._off_stage[idx % 2]
            with torch.cuda.stream(us):
                # uploads and downloads run on SEPARATE streams so PCIe
                # runs full duplex (13B sweep measured 5.7 s one-stream);
                # buffer reuse waits the previous D2H of this buffer
                if idx >= 2:
                    us.wait_event(st["d2h_done"])
                st["master"][:l].copy_(self.master[c0:c1], non_blocking=True)
                st["m"][:l].copy_(self.exp_avg[c0:c1], non_blocking=True)
                st["v"][:l].copy_(self.exp_avg_sq[c0:c1], non_blocking=True)
                st["h2d"].record(us)
            cur.wait_event(st["h2d"])
            ops.fused_adamw(
                st["master"][:l], gshard[c0:c1], st["m"][:l], st["v"][:l],
                lr=lr, beta1=cfg.beta1, beta2=cfg.beta2, eps=cfg.eps,
                weight_decay=cfg.weight_decay, step=self.step_count,
                bf16_out=param_shard[c0:c1], grad_scale=gscale,
            )
            st["done"].record(cur)
            with torch.cuda.stream(ds):
                ds.wait_event(st["done"])
                self.master[c0:c1].copy_(st["master"][:l], non_blocking=True)
                self.exp_avg[c0:c1].copy_(st["m"][:l], non_blocking=True)
                self.exp_avg_sq[c0:c1].copy_(st["v"][:l], non_blocking=True)
                st["d2h_done"].record(ds)
        # states must be home before checkpoint/next step
        cur.wait_stream(ds)
        cur.wait_stream(us)

    # ------------------------------------------------------------------
    def state_dict(self):
        return {
            "step": self.step_count,
            "master": self.master,
            "exp_avg": self.exp_avg,
            "exp_avg_sq": self.exp_avg_sq,
        }

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        self.master.copy_(sd["master"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
