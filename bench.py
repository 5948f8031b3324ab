#!/usr/bin/env python3
"""Flagship benchmark: PPO samples/sec, 4 x LLaMA-7B (actor/critic/ref/RM).

Implements the BASELINE.json metric: the reference config is
examples/scripts/local/ppo.sh (prompt len 128, train_bs_n_seqs 128 on 8
GPUs -> 16 seqs/GPU weak scaling, gen len fixed 512, top_p 0.9 / top_k
1000, 4 PPO minibatches), synthetic prompts, random-init weights, bf16.

Run:  python bench.py [--gpus N] [--steps K] [--warmup W]
          [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times K steps and prints one JSON result
line; anything else the benchmark may measure belongs behind --full.
Multi-GPU (driver):  python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...
One process per GPU over RCCL; per-model data parallelism (weak scaling:
per-GPU batch fixed at 16 sequences).
"""
import argparse
import json
import os
import time

# avoid allocator fragmentation at the 270+ GiB working set
os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")
# pre-tuned hipBLASLt/rocBLAS GEMM solutions for the bench shapes (gfx950)
_TUNED = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "realhf_amd", "data", "tunableop_gfx950.csv")
if os.path.exists(_TUNED) and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:
    # TunableOp appends the device ordinal before .csv on read — stage a
    # copy per possible ordinal in a per-user temp directory (a fixed name
    # shared by all users cannot be replaced by the second user to run).
    # All torchrun ranks execute this concurrently: copy to a rank-unique
    # temp then os.replace (atomic on POSIX) so no rank ever reads a
    # half-written CSV.
    import shutil as _sh
    import tempfile as _tf

    _stage = os.path.join(_tf.gettempdir(), f"realhf_amd_{os.getuid()}")
    os.makedirs(_stage, mode=0o700, exist_ok=True)
    _pid = os.getpid()
    for _d in range(8):
        _tmp = os.path.join(_stage, f"tunableop{_d}.csv.{_pid}")
        _sh.copy(_TUNED, _tmp)
        os.replace(_tmp, os.path.join(_stage, f"tunableop{_d}.csv"))
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = os.path.join(
        _stage, "tunableop.csv")

# sum dQ of the attention backward in a fixed order, so that two runs with
# the same arguments compute the same step bit for bit (--dump-outputs).
# A/B, 6 timed steps, two runs each: 4395-4409 ms/step with it, 4388-4395
# with atomics (REALHF_AMD_ATTN_BWD_DET=0) -- inside the run-to-run spread
os.environ.setdefault("REALHF_AMD_ATTN_BWD_DET", "1")

import numpy as np
import torch
import torch.distributed as dist


def log(msg):
    r = int(os.environ.get("RANK", "0"))
    print(f"[bench rank{r}] {msg}", flush=True, file=__import__("sys").stderr)


# --dump-outputs: elements kept per array (larger arrays are sampled) and
# the hard cap on everything written
_DUMP_MAX_ELEMS = 2 * 2**20
_DUMP_MAX_BYTES = 64 * 2**20


def dump_outputs(out_dir, sample, astats, cstats, params, first):
    """Write what the last timed step returned as out_dir/<name>.npy.

    rollout_<key>: every tensor of the step's rollout batch (generated
    sequences, logprobs, masks, rewards, ref logprobs, values);
    actor_stats / critic_stats: the train_step stat dicts as float64
    vectors in sorted-key order (names in manifest.json);
    <role>_params: the updated flat parameters;
    first_rollout_<key>: the rollout batch of the very first step executed
    (warmup included), i.e. computed from the initial weights alone.
    Arrays are float32 in their own shape; one larger than
    _DUMP_MAX_ELEMS is flattened and reduced to a fixed sample whose
    indices are seeded by the array's name, so two runs pick the same
    elements.
    """
    import zlib

    os.makedirs(out_dir, exist_ok=True)
    manifest = {}
    total = 0

    def save(name, arr, **extra):
        nonlocal total
        total += arr.nbytes
        assert total <= _DUMP_MAX_BYTES, (name, total)
        np.save(os.path.join(out_dir, name + ".npy"), arr)
        manifest[name] = dict(shape=list(arr.shape), dtype=str(arr.dtype),
                              **extra)

    def save_tensor(name, t):
        t = t.detach()
        extra = {}
        if t.numel() > _DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.randint(0, t.numel(), (_DUMP_MAX_ELEMS,), generator=g)
            extra = dict(sampled_from=list(t.shape), sample_seed=g.initial_seed())
            t = t.reshape(-1)[idx.to(t.device)]
        save(name, t.to(torch.float32).cpu().numpy(), **extra)

    for k in sorted(sample.keys):
        save_tensor("rollout_" + k, sample.data[k])
    for name, stats in (("actor_stats", astats), ("critic_stats", cstats)):
        keys = sorted(stats)
        save(name, np.array([float(stats[k]) for k in keys], dtype=np.float64),
             keys=keys)
    for role, flat in params.items():
        save_tensor(role + "_params", flat)
    for k in sorted(first):
        save_tensor("first_rollout_" + k, first[k])
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    log(f"dumped {len(manifest)} arrays ({total / 2**20:.1f} MiB) to {out_dir}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seqs-per-gpu", type=int, default=16)
    p.add_argument("--prompt-len", type=int, default=128)
    p.add_argument("--gen-len", type=int, default=512)
    p.add_argument("--n-minibatches", type=int, default=4)
    p.add_argument("--model", type=str, default="llama-7b",
                   help="llama-7b | llama-small (debug)")
    p.add_argument("--no-hip-graph", action="store_true")
    p.add_argument("--phase-timing", action="store_true",
                   help="per-phase sync+timing (serializes side-stream overlap)")
    p.add_argument("--no-offload-frozen", dest="offload_frozen",
                   action="store_false", default=True)
    p.add_argument("--offload-set", type=str, default="",
                   help="comma list of frozen roles to offload.  Default "
                        "NONE since round 2: 4x7B fits 265.6 GiB resident "
                        "on 288 GB, and the A/B measured 3.67 samples/s "
                        "resident vs 3.50 offloaded (reload copyBuffer "
                        "traffic was 15%% of GPU time in rocprof) — "
                        "offload pays only when memory forces it (70B "
                        "tier, or --offload-set ref,rew)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step returned (rollout tensors, train stats, a "
                        "seeded sample of the updated actor/critic "
                        "parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement or check "
                        "that needs runs of its own.  The benchmark has "
                        "none today; a plain run does only setup, warmup, "
                        "the timed steps and the result line")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus or world == 1, (world, args.gpus)

    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank)
        device = torch.device(f"cuda:{local_rank}")
    else:  # CPU debug path (--model llama-small); the driver always has GPUs
        device = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl" if use_cuda else "gloo",
                                rank=rank, world_size=world)

    import realhf_amd.interfaces  # noqa: F401
    import realhf_amd.models.hf  # noqa: F401
    import realhf_amd.runtime.engine  # noqa: F401
    from realhf_amd.api.config import Abstraction, ModelName
    from realhf_amd.api.data import SequenceSample
    from realhf_amd.api.model import (
        FinetuneSpec,
        Model,
        make_backend,
        make_interface,
    )
    from realhf_amd.base import constants, seeding
    from realhf_amd.base.topology import ParallelGrid, PipeDataTensorTopology
    from realhf_amd.models.hf.llama import llama7b_config, make_test_config
    from realhf_amd.models.real_model import ReaLModel

    # model weights must be IDENTICAL across DP replicas; per-rank
    # divergence only for data/sampling (below)
    seeding.set_random_seed(1234, rank_offset=0)

    def mkcfg(is_critic):
        if args.model == "llama-7b":
            return llama7b_config(is_critic=is_critic)
        cfg = make_test_config(
            n_layers=4, hidden_dim=512, n_heads=8, n_kv_heads=8,
            head_dim=64, intermediate_dim=1408, vocab_size=32000,
            max_position_embeddings=2048, is_critic=is_critic,
        )
        cfg.family = "llama"
        return cfg

    # grids: every model spans all ranks, pure DP (round-1 allocation)
    names = ["actor", "critic", "ref", "rew"]
    if world > 1:
        for n in names:
            topo = PipeDataTensorTopology(num_pp=1, num_dp=world, num_tp=1)
            constants.set_grid(n, ParallelGrid(topo))

    def scope(n):
        import contextlib

        if constants.has_model(n):
            return constants.model_scope(n)
        return contextlib.nullcontext()

    log("building models (4x %s, bf16, random init)..." % args.model)
    t0 = time.time()
    models = {}
    for n in names:
        is_critic = n in ("critic", "rew")
        cfg = mkcfg(is_critic)
        with scope(n):
            m = ReaLModel(cfg, device=device,
                          dtype=torch.bfloat16 if use_cuda else torch.float32)
            # zlib.crc32, NOT hash(): python str hashes are salted per
            # process, which would give each DP rank different weights
            import zlib

            torch.manual_seed(4242 + zlib.crc32(n.encode()) % 1000)
            m.random_init()
            model = Model(
                name=ModelName(n, 0), module=m, tokenizer=None, device=device,
                dtype=torch.bfloat16,
            )
            if n in ("actor", "critic"):
                backend = make_backend(
                    Abstraction("zero1", {"optimizer": {"lr": 1e-6,
                                                        "warmup_steps_proportion": 0.0}})
                )
            else:
                backend = make_backend(Abstraction("inference"))
            models[n] = backend.initialize(model, FinetuneSpec(1, 512, 128))
        if use_cuda:
            torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated() / 2**30 if use_cuda else 0.0
    log(f"models built in {time.time() - t0:.1f}s; mem={mem:.1f} GiB")

    # DP replicas must start from identical weights (weak-scaling
    # validity): verify with a cheap checksum all-reduce
    if world > 1:
        for n in names:
            with scope(n):
                mm = models[n].module.module
                cs = mm.flat_param.float().sum()
                lo, hi = cs.clone(), cs.clone()
                dist.all_reduce(lo, op=dist.ReduceOp.MIN)
                dist.all_reduce(hi, op=dist.ReduceOp.MAX)
                assert torch.allclose(lo, hi, rtol=1e-5), (
                    f"{n}: DP replicas differ at init ({lo} vs {hi})")

    gconfig = dict(
        max_new_tokens=args.gen_len, min_new_tokens=args.gen_len,
        greedy=False, top_k=1000, top_p=0.9, temperature=1.0,
        use_hip_graph=not args.no_hip_graph and torch.cuda.is_available(),
    )
    actor_iface = make_interface(
        Abstraction("ppo_actor", {
            "n_minibatches": args.n_minibatches, "gconfig": gconfig,
            "kl_ctl": 0.1, "adv_norm": True,
            # actor_train is followed by critic_train: the final param
            # all-gather hides under it (waited at next generate)
            "defer_final_allgather": world > 1,
        })
    )
    critic_iface = make_interface(
        Abstraction("ppo_critic", {
            "n_minibatches": args.n_minibatches,
            # critic_train is the LAST phase of the step: its final
            # param all-gather hides under the NEXT step's generation
            # (engines wait it before any param use)
            "defer_final_allgather": world > 1,
        })
    )
    rew_iface = make_interface(Abstraction("paired_rw"))

    vocab = models["actor"].module.module.config.vocab_size
    rng = np.random.RandomState(1000 + rank)

    def make_prompt_batch():
        bs = args.seqs_per_gpu
        toks = torch.from_numpy(
            rng.randint(10, vocab - 10, size=bs * args.prompt_len)
        ).long().to(device)
        return SequenceSample(
            keys=("packed_prompts",),
            ids=[f"r{rank}-{i}" for i in range(bs)],
            seqlens={"packed_prompts": [[args.prompt_len]] * bs},
            data={"packed_prompts": toks},
        )

    frozen = tuple(r for r in args.offload_set.split(",") if r) \
        if args.offload_frozen else ()

    phase_t = {}

    def mark(name, t0):
        if not args.phase_timing:
            return t0
        if use_cuda:
            torch.cuda.synchronize()
        now = time.time()
        phase_t[name] = phase_t.get(name, 0.0) + (now - t0)
        return now

    def ppo_step():
        t = time.time()
        batch = make_prompt_batch()
        # prefetch the reward model's weights: H2D overlaps generation
        if "rew" in frozen:
            models["rew"].module.model.start_reload()
        with scope("actor"):
            rollout = actor_iface.generate(models["actor"], batch)
        t = mark("actor_gen", t)
        sample = rollout
        seq_only = sample.select_keys(["packed_input_ids"])
        with scope("rew"):
            if "rew" in frozen:
                models["rew"].module.model.reload_from_offload()
                t = mark("rew_reload", t)
            if "ref" in frozen:
                models["ref"].module.model.start_reload()  # overlap rew_inf
            sample.update_(rew_iface.inference(models["rew"], seq_only))
            if "rew" in frozen:
                models["rew"].module.model.async_offload()
        t = mark("rew_inf", t)
        with scope("ref"):
            if "ref" in frozen:
                models["ref"].module.model.reload_from_offload()
                t = mark("ref_reload", t)
            sample.update_(actor_iface.inference(models["ref"], seq_only))
            if "ref" in frozen:
                models["ref"].module.model.async_offload()
        t = mark("ref_inf", t)
        with scope("critic"):
            sample.update_(critic_iface.inference(models["critic"], seq_only))
        t = mark("critic_inf", t)
        with scope("actor"):
            astats = actor_iface.train_step(models["actor"], sample)
        t = mark("actor_train", t)
        with scope("critic"):
            cstats = critic_iface.train_step(models["critic"], sample)
        t = mark("critic_train", t)
        return astats, cstats, sample

    for n in frozen:
        models[n].module.model.async_offload()

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    log(f"warmup x{args.warmup}...")
    # --dump-outputs keeps the rollout batch of the first executed step
    # (copied: it is computed from the initial weights alone) and a
    # reference to the last one; a plain run keeps neither
    first_rollout = rollout = None

    def copy_rollout(sample):
        return {k: sample.data[k].detach().clone() for k in sample.keys}

    for i in range(args.warmup):
        rollout = ppo_step()[2]
        if args.dump_outputs and first_rollout is None:
            first_rollout = copy_rollout(rollout)
        rollout = None
        m2 = torch.cuda.max_memory_allocated() / 2**30 if use_cuda else 0.0
        log(f"warmup step {i} done; peak mem={m2:.1f} GiB")
    barrier_sync()

    phase_t.clear()
    t0 = time.time()
    for i in range(args.steps):
        astats, cstats, rollout = ppo_step()
        if not args.dump_outputs:
            rollout = None
        elif first_rollout is None:  # --warmup 0: no earlier place for it
            first_rollout = copy_rollout(rollout)
        log(f"step {i}: actor_loss={astats.get('actor_loss', 0):.4f} "
            f"kl={astats.get('kl', 0):.4f}")
    barrier_sync()
    elapsed = time.time() - t0
    if args.phase_timing:
        log("phase breakdown (s/step): " + json.dumps(
            {k: round(v / args.steps, 3) for k, v in phase_t.items()}))

    # MAX elapsed over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)

    # DP replicas must still agree after the timed steps (guards the
    # bucketed ZeRO overlap path: a mis-ordered reduce-scatter would
    # silently diverge the replicas and invalidate the number)
    if world > 1:
        for n in ("actor", "critic"):
            models[n].module.optimizer.finish_allgather()
        for n in ("actor", "critic"):
            with scope(n):
                mm = models[n].module.module
                cs = mm.flat_param.float().sum()
                lo, hi = cs.clone(), cs.clone()
                dist.all_reduce(lo, op=dist.ReduceOp.MIN)
                dist.all_reduce(hi, op=dist.ReduceOp.MAX)
                assert torch.allclose(lo, hi, rtol=1e-6, atol=0), (
                    f"{n}: DP replicas diverged after training ({lo} vs {hi})")

    if args.dump_outputs and rank == 0:
        with torch.no_grad():
            dump_outputs(
                args.dump_outputs, rollout, astats, cstats,
                {n: models[n].module.module.flat_param
                 for n in ("actor", "critic")},
                first_rollout)

    n_gpus = world
    total_samples = args.seqs_per_gpu * n_gpus * args.steps
    samples_per_sec = total_samples / elapsed
    ms_per_step = elapsed / args.steps * 1000

    if rank == 0:
        result = {
            "metric": "PPO samples/sec (whole node), 4xLLaMA-7B actor/critic/ref/RM",
            "value": samples_per_sec,
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": "4x" + args.model,
                "global_batch": args.seqs_per_gpu * n_gpus,
                "seq_len": args.prompt_len + args.gen_len,
                "prompt_len": args.prompt_len,
                "gen_len": args.gen_len,
                "parallelism": f"dp{n_gpus}",
                "ppo_n_minibatches": args.n_minibatches,
            },
        }
        print(json.dumps(result), flush=True)

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
