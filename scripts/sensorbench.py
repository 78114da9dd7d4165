"""What the per-env sensor model (observation latency and bias; csrc/nm_sensor.h) costs the one-launch rollout, switched off and on.

env-steps/s of policy_rollout (nm_rollout, the reference's 66 -> 54 -> 42 -> 30 -> 18 | 1 networks) at N envs x T steps (default
4096 x 80) in three configurations:
    parent   another build of the library (--parent-lib: the parent commit's libnightmare_hip.so), which has no sensor hook
    off      this tree, the model off: the hook is one wave-uniform branch per step
    on       this tree, delays drawn in 0..3 for both groups and a bias on every kind
Every measurement is a child process of its own (a fresh HIP context; this process never touches the GPU): WARMUP launches, then REPS
launches timed one by one with HIP events; the figure is N x T over the median launch time. The configurations alternate parent, off,
on, parent, ... RUNS times, so that a drift of the machine shows in all columns, and the off figure is judged against the spread of the
parent's own repeated runs in this session. A fourth child times the per-step path: step() with the model off and on in alternating
blocks; the difference per step is k_sensor (one small launch behind k_env_step).

  python scripts/sensorbench.py [N] [T] [--runs 3] [--reps 30] [--parent-lib PATH] [--out profiles/sensorbench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = dict(lin_vel=0.2, ang_vel=0.05, gravity=0.02, dof_pos=0.03, dof_vel=0.1)      # observation units


def _env(N):
    import torch
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    env = NightmareV3Env(cfg, device="cuda:0", seed=1)
    env.reset()
    torch.manual_seed(3)
    env.episode_length_buf = torch.randint(0, int(env.max_episode_length), (N,), device="cuda:0", dtype=torch.int64)
    return env


def child_rollout(a):
    sys.path.insert(0, ROOT)
    import torch
    from nightmare_rl_amd import _lib
    from nightmare_rl_amd.rl import ActorCritic, RolloutStorage
    from nightmare_rl_amd.rl.fused import FusedUpdate
    dev, N, T = "cuda:0", a.N, a.T
    env = _env(N)
    if a.child == "on":
        env.draw_sensor_model((0, 3), (0, 3), BIAS)
    torch.manual_seed(5)
    ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu", init_noise_std=0.8).to(dev)
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
    st = RolloutStorage(N, T, [66], [None], [18], dev)
    z = lambda n: torch.zeros(n, device=dev)
    cur_ret, cur_len, fin, lv = z(N), z(N), z(3), z(N)
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    ms = []
    for rep in range(a.warmup + a.reps):
        it.fill_(rep)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        env.policy_rollout(T, fu.flat, 99, it, st, 0.99, cur_ret, cur_len, fin, last_values=lv)
        e1.record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    on = bool(env.sensor_model()["on"]) if hasattr(env._L, "nm_set_sensor") else False
    print(json.dumps(dict(config=a.child, lib=_lib.LIB_PATH, sensor_on=on, launch_ms=ms, median_ms=med, env_steps_per_s=N * T / (med * 1e-3),
                          finite=bool(torch.isfinite(st.observations).all()))), flush=True)
    env.close()


def child_step(a):
    sys.path.insert(0, ROOT)
    import torch
    N, steps = a.N, 200
    env = _env(N)
    act = torch.zeros((N, 18), device="cuda:0")
    per = {"off": [], "on": []}
    for block in range(2 * 6):
        mode = "on" if block % 2 else "off"
        if mode == "on":
            env.draw_sensor_model((0, 3), (0, 3), BIAS)
        else:
            env.set_sensor_model(None, None, None)
        for _ in range(20):
            env.step(act)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            env.step(act)
        e1.record()
        torch.cuda.synchronize()
        if block >= 2:
            per[mode].append(e0.elapsed_time(e1) * 1e3 / steps)
    off, on = statistics.median(per["off"]), statistics.median(per["on"])
    print(json.dumps(dict(config="step", step_us_off=per["off"], step_us_on=per["on"], median_off_us=off, median_on_us=on, k_sensor_us=on - off)), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int, nargs="?", default=4096)
    ap.add_argument("T", type=int, nargs="?", default=80)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("parent", "off", "on", "step"), default=None)
    a = ap.parse_args()
    if a.child == "step":
        return child_step(a)
    if a.child:
        return child_rollout(a)
    configs = (["parent"] if a.parent_lib else []) + ["off", "on"]
    res = {c: [] for c in configs}
    raw = []

    def run(c):
        env = dict(os.environ)
        env.pop("NM_HIP_LIB", None)
        if c == "parent":
            env["NM_HIP_LIB"] = os.path.abspath(a.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), str(a.N), str(a.T), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child", c]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300, env=env)
        if out.returncode != 0:      # nothing more is started on the device after a child that failed
            raise SystemExit(f"{c}: child left with status {out.returncode}")
        return json.loads(out.stdout.strip().splitlines()[-1])

    for r in range(a.runs):
        for c in configs:
            d = run(c)
            if d["sensor_on"] != (c == "on") or not d["finite"]:
                raise SystemExit(f"run {r} {c}: sensor_on {d['sensor_on']}, finite {d['finite']}")
            res[c].append(d["env_steps_per_s"])
            raw.append(d)
            print(f"run {r} {c:6s} ({os.path.basename(d['lib'])}): {a.N} x {a.T}: median launch {d['median_ms']:.3f} ms = {d['env_steps_per_s'] / 1e6:.3f} M env-steps/s", flush=True)
    step = run("step")
    print(f"per-step path at {a.N} envs: step() {step['median_off_us']:.2f} us with the model off, {step['median_on_us']:.2f} us on: k_sensor {step['k_sensor_us']:.2f} us per step")
    summary = {c: dict(runs=v, median=statistics.median(v), lo=min(v), hi=max(v)) for c, v in res.items()}
    for c, s in summary.items():
        print(f"{c:6s} {s['lo'] / 1e6:.3f} .. {s['hi'] / 1e6:.3f} M env-steps/s (median {s['median'] / 1e6:.3f}, spread {(s['hi'] - s['lo']) / s['median'] * 100:.2f} %)")
    if a.parent_lib:
        p, o = summary["parent"], summary["off"]
        inside = p["lo"] <= o["median"] <= p["hi"] or o["median"] >= p["lo"]
        print(f"off against parent: ratio of medians {o['median'] / p['median']:.4f}; the off median lies "
              f"{'inside or above' if inside else 'BELOW'} the parent's own spread [{p['lo'] / 1e6:.3f}, {p['hi'] / 1e6:.3f}]")
        print(f"on against off: ratio of medians {summary['on']['median'] / o['median']:.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(N=a.N, T=a.T, runs=a.runs, reps=a.reps, warmup=a.warmup, summary=summary, step=step, children=raw), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
