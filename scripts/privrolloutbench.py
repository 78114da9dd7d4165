"""Collection of one PPO iteration with privileged critic observations (cfg.env.privileged_obs; actor 66 -> 54 -> 42 -> 30 -> 18, critic
89 -> 54 -> 42 -> 30 -> 1) at N envs x T steps (default 4096 x 80): the one-launch rollout (nm_rollout_priv; runner option
privileged_rollout) against the per-step collection (nm_policy_forward, nm_ppo_sample_prefix, nm_ppo_record, the env step and k_priv_obs
per step - captured into a graph by the runner where it can be).

Every run is a child process of its own (a fresh HIP context; the parent process never touches the GPU): OnPolicyRunner.learn for ITERS
iterations, and the runner's `collection_time` (HIP events around the rollout) of the last ITERS - 3 of them. The runs alternate
per-step, one-launch, per-step, ... RUNS times, so that a drift of the machine shows in both columns. The update is the generic fused update in
both; it is not what is measured.

  python scripts/privrolloutbench.py [N] [T] [--runs 3] [--iters 8] [--rows] [--baseline-tree DIR]

--rows               per-env friction and payload rows drawn at construction (cfg.domain_rand): the level-2 step instead of level 0
--baseline-tree DIR  take the per-step runs from the package in DIR (a built checkout of another revision) instead of this one: the
                     comparison against that revision's collection in the same session"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.tree)
    import torch
    from nightmare_rl_amd import _lib
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    from nightmare_rl_amd.rl import OnPolicyRunner

    class PrivConfig(NightmareV3Config):
        class env(NightmareV3Config.env):
            privileged_obs = True

    class domain_rand:
        randomize_friction, friction_range = True, (0.5, 1.25)
        randomize_base_mass, added_mass_range = True, (-0.2, 0.4)

    cfg = PrivConfig()
    cfg.env.num_envs = a.N
    if a.rows:
        cfg.domain_rand = domain_rand
    torch.manual_seed(0)
    env = NightmareV3Env(cfg, device="cuda:0", seed=1)
    tc = class_to_dict(NightmareV3ConfigPPO())
    tc["runner"]["save_interval"] = 10 ** 9
    tc["runner"]["num_steps_per_env"] = a.T
    tc["runner"]["privileged_rollout"] = a.child == "one-launch"
    r = OnPolicyRunner(env, tc, log_dir=None, device="cuda:0")
    r.learn(a.iters, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    c = [h["collection_time"] * 1e3 for h in r.history[3:]]
    print(json.dumps(dict(mode=a.child, lib=_lib.LIB_PATH, rollout_mode=r.rollout_mode, collection_ms=c, median_ms=statistics.median(c),
                          value_loss=r.history[-1]["value_loss"])), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int, nargs="?", default=4096)
    ap.add_argument("T", type=int, nargs="?", default=80)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--child", choices=("per-step", "one-launch"), default=None)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.iters < 4:
        ap.error("--iters must be at least 4 (the first three iterations are warm-up)")
    if a.child:
        return child(a)
    res = {"per-step": [], "one-launch": []}
    for run in range(a.runs):
        for mode in ("per-step", "one-launch"):
            tree = os.path.abspath(a.baseline_tree) if (mode == "per-step" and a.baseline_tree) else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), str(a.N), str(a.T), "--iters", str(a.iters), "--child", mode, "--tree", tree] + (["--rows"] if a.rows else [])
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
            if out.returncode != 0:      # nothing more is started on the device after a child that failed
                raise SystemExit(f"run {run} {mode}: child left with status {out.returncode}")
            d = json.loads(out.stdout.strip().splitlines()[-1])
            want = "one launch (nm_rollout, privileged)" if mode == "one-launch" else "per-step launches"
            if d["rollout_mode"] != want:
                raise SystemExit(f"run {run} {mode}: the runner collected through {d['rollout_mode']!r}")
            res[mode].append(d["median_ms"])
            print(f"run {run} {mode:10s} ({os.path.relpath(d['lib'])}): collection {a.N} x {a.T}{' with rows' if a.rows else ''}: median {d['median_ms']:.3f} ms; "
                  + " ".join(f"{x:.3f}" for x in d["collection_ms"]), flush=True)
    p, o = res["per-step"], res["one-launch"]
    print(f"per-step   {min(p):.3f} .. {max(p):.3f} ms (spread {max(p) - min(p):.3f})")
    print(f"one-launch {min(o):.3f} .. {max(o):.3f} ms (spread {max(o) - min(o):.3f})")
    print(f"one launch faster in every run: {all(x < y for x, y in zip(o, p))}; ratio of medians {statistics.median(p) / statistics.median(o):.3f}")


if __name__ == "__main__":
    main()
