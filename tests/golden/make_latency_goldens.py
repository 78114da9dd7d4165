"""Generator of tests/golden/latency.npz: fp64 reference trajectories for per-env actuation latency (nm_set_action_latency).

The oracle keeps, per env, a delay d in substeps and the last H = 3 scaled and clipped float actions (oracle/nm_oracle.h:
OracleEnv.set_action_latency, hist[j] = a_{t-1-j}); with k = d / DECIMATION, r = d % DECIMATION a step runs r substeps under the command
of a_{t-k-1}, then DECIMATION - r under that of a_{t-k} (a_t itself where k = 0), each command being the step's own expression on the
same dof_pos snapshot; then it shifts the history. Everything else of the step (observation, rewards, action buffers) keeps a_t.

The script first asserts that delay 0 set in every env equals no delays set at all bit for bit over both populations, then records,
free-running (every step's start state is the previous step's end state), with the delays DELAYS over the eight envs:
    drop   random actions while the robot falls from the initial pose and lands
    stand  small random actions, new every step, after the robot has settled on its feet under such actions
Nothing but the .npz is written into the tree.

    python tests/golden/make_latency_goldens.py            (CPU only, a few seconds)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "latency.npz")
DELAYS = np.array([0, 1, 2, 3, 4, 5, 6, 0], np.int32)      # a two-env wave (2w, 2w + 1) always holds two different switch substeps r
POPS = ("drop", "stand")
N, T, H = 8, 10, 3
SEED = 5
KEYS = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "hist", "actions", "cmd_u", "obs", "rew", "done", "ncon")
sys.path.insert(0, ROOT)
from oracle import oracle as orc      # noqa: E402


def record(delays, window=None, extra_keys=()):
    """One free-running recording of both populations under one action stream. delays: [N] or None = never set. window(o, past) is
    called where a recorded window starts, with the scaled and clipped actions of the pre-roll (the oracle's own buffer after each step):
    make_servo_goldens.py switches its model on there and records `lim` besides."""
    rng = np.random.default_rng(SEED)
    res = {}
    for pop in POPS:
        o = orc.OracleEnv(N, seed=SEED)
        if delays is not None:
            o.set_action_latency(delays)        # a fresh, zero history
        o.reset_idx()
        if pop == "drop":
            pre, act = 7, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        else:
            pre, act = 150, lambda: rng.uniform(-0.12, 0.12, (N, 18)).astype(np.float32)
        past = []
        for _ in range(pre):
            o.step(act())
            past.append(o.get_buffers()["actions"].copy())
        if window:
            window(o, past)
        r = {k: [] for k in KEYS + tuple(extra_keys)}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"])
            r["hist"].append(o.action_history()[0])
            if "lim" in r:
                r["lim"].append(o.servo_state()[1])

        state()
        for t in range(T):
            a = act()
            cu = rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            state()
        for k in r:
            res[f"{pop}_{k}"] = np.stack(r[k])
    return res


def main():
    plain, zero, g = record(None), record(np.zeros(N, np.int32)), record(DELAYS)
    for key in plain:        # delay 0 changes nothing
        np.testing.assert_array_equal(plain[key], zero[key], err_msg=key)
    print("delay 0 in every env equals no delays set bit for bit")
    g["delays"] = DELAYS
    for pop in POPS:
        moved = np.abs(g[f"{pop}_qpos"] - zero[f"{pop}_qpos"]).max(axis=(0, 2))
        print(f"{pop}: env-steps with contacts {(g[f'{pop}_ncon'] > 0).sum()} of {N * T}, resets {int(g[f'{pop}_done'].sum())}, "
              f"max |qpos - undelayed qpos| per env {np.array2string(moved, precision=2)}")
        assert (moved[DELAYS > 0] > 1e-6).all() and (moved[DELAYS == 0] == 0).all(), "a delayed env must differ from its undelayed run, an undelayed one must not"
        # the recorded histories are the recorded actions, scaled and clipped by the oracle (its actions buffer)
        np.testing.assert_array_equal(g[f"{pop}_hist"][1:, :, 0], g[f"{pop}_act"][1:].astype(np.float32))
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
