"""bench.py command line: result line fields, --full, --dump-outputs.

Runs the benchmark's CPU debug configuration (--model llama-small) in a
child process with the GPUs hidden, so it needs no device."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--model", "llama-small", "--seqs-per-gpu", "4",
         "--prompt-len", "8", "--gen-len", "8"]


def _run_bench(*extra):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout  # exactly one JSON result line
    return json.loads(lines[0]), out.stderr


def test_bench_dump_outputs_repeatable(tmp_path):
    """Two runs with the same arguments see the same inputs and write the
    same arrays; --steps sets the number of timed steps."""
    res, err = _run_bench("--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "a"))
    assert res["steps"] == 2 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 4 / (res["ms_per_step"] / 1000)) < 1e-6 * res["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in res
    # one log line per timed step, none for steps that were not asked for
    assert "] step 1:" in err and "] step 2:" not in err

    _run_bench("--steps", "2", "--warmup", "1", "--full",
               "--dump-outputs", str(tmp_path / "b"))
    names = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert {"rollout_packed_input_ids.npy", "rollout_packed_logprobs.npy",
            "rollout_rewards.npy", "rollout_values.npy", "actor_stats.npy",
            "critic_stats.npy", "actor_params.npy",
            "critic_params.npy",
            "first_rollout_packed_input_ids.npy"} <= set(names)
    total = 0
    for f in names:
        a = np.load(tmp_path / "a" / f)
        b = np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 * 2**20
    ids = np.load(tmp_path / "a" / "rollout_packed_input_ids.npy")
    assert ids.shape == (4 * 16,)
    # the first step's rollout is a different batch (new prompts, and the
    # weights have been updated in between), not a copy of the last one
    first = np.load(tmp_path / "a" / "first_rollout_packed_input_ids.npy")
    assert first.shape == ids.shape and not np.array_equal(first, ids)
    manifest = json.load(open(tmp_path / "a" / "manifest.json"))
    assert "actor_loss" in manifest["actor_stats"]["keys"]
    assert manifest["actor_params"]["sampled_from"]
