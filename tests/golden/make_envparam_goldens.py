"""Generator of tests/golden/env_params.npz: fp64 reference trajectories for per-env friction and servo gains (mu, p_gain, kv).

The oracle carries the three values as per-env rows (oracle/nm_oracle.h: OracleEnv.set_env_params): for each parameter set this script
gives all eight envs of an env object that row and records. Nothing but the .npz is written into the tree.

    python tests/golden/make_envparam_goldens.py            (CPU only, a few seconds)

Populations (8 envs x T steps each, per set, free-running; every step's start state is the previous step's end state):
    drop   random actions while the robot falls from the initial pose and lands
    stand  zero actions after the robot has settled on its feet
    belly  the robot lying on folded legs while its servos hold the pose (the initial states of env_manycontacts.npz): of 80 steps the T
           consecutive ones with the most env-steps above 16 contacts (the matrix-free constraint layout)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "env_params.npz")
# each value differs from the default (1, 20, 0.8) in at least one set, and in both directions
SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])
POPS = ("drop", "stand", "belly")
N, T = 8, 10
SEED = 5
KEYS = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon")
sys.path.insert(0, ROOT)
from oracle import oracle as orc      # noqa: E402


def record(setup=None, pops=POPS, lib_path=None, extra=None):
    """One free-running recording of the populations `pops`, in this order under one action stream. setup(o) gives a fresh env object
    its rows; lib_path binds another library (a base payload is a recompiled model); extra(o) returns more per-step keys and is first
    called, its result dropped, where a recorded window starts. Shared by the generators of payload, gravity, torque and wrench."""
    rng = np.random.default_rng(SEED)
    res = {}
    many = np.load(os.path.join(HERE, "env_manycontacts.npz"))["init_qpos"][:N]
    default = np.tile([0, np.pi / 5, 0], 6)
    for pop in pops:
        o = orc.OracleEnv(N, seed=SEED, lib_path=lib_path)
        o.reset_idx()
        if setup:
            setup(o)
        if pop == "drop":
            pre, act = 7, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        elif pop == "stand":
            pre, act = 150, lambda: np.zeros((N, 18), np.float32)
        else:
            o.set_state(many, np.zeros((N, 24)), np.zeros((N, 24)))
            o.set_buffers(dof_pos=many[:, 7:])
            pre, act = 0, lambda: np.clip((o.get_buffers()["dof_pos"] + default) / 0.2, -5, 5).astype(np.float32)
        total = T if pop != "belly" else 80       # belly: the T consecutive steps with the most env-steps above 16 contacts are kept
        for _ in range(pre):
            o.step(act())
        more = extra(o) if extra else {}
        keys = KEYS + tuple(more)
        r = {k: [] for k in keys}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"])

        state()
        for t in range(total):
            a = act()
            cu = rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            for k, v in (extra(o) if extra else {}).items():
                r[k].append(v)
            state()
        big = (np.stack(r["ncon"]) > 16).sum(axis=1)
        t0 = int(np.argmax([big[i:i + T].sum() for i in range(total - T + 1)]))
        for k in keys:
            res[f"{pop}_{k}"] = np.stack(r[k][t0:t0 + T + (len(r[k]) > total)])
    return res


def stacked(parts):
    """[set, step (T or T + 1), env, ...] per key."""
    return {key: np.stack([p[key] for p in parts]) for key in parts[0]}


def main():
    parts = [record(lambda o, row=row: o.set_env_params(row)) for row in SETS]
    g = {"sets": SETS, **stacked(parts)}
    for pop in POPS:
        big = (g[f"{pop}_ncon"] > 16).sum(axis=(1, 2))
        con = (g[f"{pop}_ncon"] > 0).sum(axis=(1, 2))
        print(f"{pop}: env-steps with contacts per set {con.tolist()}, with more than 16 contacts {big.tolist()}, resets {g[f'{pop}_done'].sum(axis=(1, 2)).tolist()}")
    assert ((g["belly_ncon"] > 16).sum(axis=(1, 2)) >= 4).all(), "every set must exercise the matrix-free layout on several env-steps"
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
