"""bench.py's plain run (headline line only) and --dump-outputs: two runs with the same arguments time the asked number of steps and
write the same outputs. Named test_00_* like test_00_bench_multirank.py: the runs are child processes started before this pytest
process touches the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_a_fixed_sample_above_the_limit(tmp_path):
    import torch
    from bench import dump_outputs
    obs = torch.arange(1000 * 66, dtype=torch.float32).reshape(1000, 66)
    arrays = {"obs": obs, "rewards": torch.arange(1000.0), "dones": torch.zeros(1000, dtype=torch.int64), "time_outs": None,
              "episode_sums": torch.ones(16)}
    dump_outputs(str(tmp_path / "all"), "", arrays)
    assert sorted(os.listdir(tmp_path / "all")) == ["dones.npy", "episode_sums.npy", "obs.npy", "rewards.npy"]
    assert np.array_equal(np.load(tmp_path / "all" / "obs.npy"), obs.numpy())
    limit = 100 * (66 + 1 + 1) * 4
    for d in ("a", "b"):
        dump_outputs(str(tmp_path / d), "_rank1", arrays, limit=limit)
    files = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(v.nbytes for v in files.values()) <= limit
    ids = files["env_ids_rank1.npy"].astype(np.int64)
    assert files["env_ids_rank1.npy"].dtype == np.float64 and len(ids) > 50 and np.all(np.diff(ids) > 0)
    assert np.array_equal(files["obs_rank1.npy"], obs.numpy()[ids]) and np.array_equal(files["rewards_rank1.npy"], ids.astype(np.float32))
    assert files["episode_sums_rank1.npy"].shape == (16,)
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f)) for f, v in files.items())      # the sample is seeded


@pytest.mark.gpu
def test_plain_bench_line_and_reproducible_outputs(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    lines, dumps = [], []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5", "--envs-per-gpu", "1024",
               "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    out = lines[0]
    assert out["steps"] == 30 and out["warmup"] == 5 and out["n_gpus"] == 1 and out["unit"] == "env-steps/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and abs(out["value"] - 1024 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"roofline", "contact_regime", "cpu_baseline", "ppo_end_to_end_env_steps_per_s"} & set(out)     # secondary legs: --full only
    a, b = dumps
    assert sorted(a) == ["dones.npy", "episode_sums.npy", "obs.npy", "returns.npy", "rewards.npy", "time_outs.npy"]
    assert a["obs.npy"].shape == (1024, 66) and all(v.dtype == np.float32 for v in a.values())
    assert np.isfinite(a["obs.npy"]).all() and np.abs(a["returns.npy"]).max() > 0
    for f in a:
        if f == "episode_sums.npy":      # float32 sums over all envs, accumulated in whatever order the waves reach them
            np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=1e-6, err_msg=f)
        else:                            # per-env outputs: bit-identical
            np.testing.assert_array_equal(a[f], b[f], err_msg=f)
