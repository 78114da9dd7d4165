"""Generator of tests/golden/payload.npz: fp64 reference trajectories for per-env base payloads (a point mass dm at r on the base body).

An env with payload (dm, r) behaves as if mjmodel.xml had been recompiled with that mass added to base_link. The oracle takes its model
from nightmare_rl_amd/model/nm_model_data.h at compile time, so a UNIFORM variant of the oracle is the unchanged oracle source compiled
against the header that compile_model.emit_header writes for the modified tables T' (nightmare_rl_amd/model/payload.py
modified_tables: body_mass / body_ipos / body_iquat / body_inertia of body 1 from eigh of I' with a right-handed axis set,
body_invweight0 and meaninertia recomputed at qpos0 through compile_model's own functions). For each payload set this script copies
oracle/*.c and oracle/nm_oracle.h into a temporary directory that mirrors the relative include path, writes that header there, builds a
library with the flags of oracle/Makefile and drives it through oracle/oracle.py in a child process (one library per process). Nothing
but the .npz is written into the tree; oracle/ itself is not touched.

    python tests/golden/make_payload_goldens.py            (CPU only, about a minute)

Populations (8 envs x T steps each, per set, free-running; every step's start state is the previous step's end state):
    drop   random actions while the robot falls from the initial pose and lands
    stand  zero actions after the robot has settled on its feet
    belly  the robot lying on folded legs while its servos hold the pose (the initial states of env_manycontacts.npz): of 80 steps the T
           consecutive ones with the most env-steps above 16 contacts (the matrix-free constraint layout)
Besides the trajectories the file holds `sets` [4,4] (dm, rx, ry, rz), `rows` [4,20] (the body rows of the four sets, by the per-env path)
and `stand_height` [4]: the mean base-body COM height of the standing population at the start of its recorded steps.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "payload.npz")
# (dm kg, r m): none, a battery forward and above, a lighter base plate, a camera mast aft - all admissible, all with distinct constants
SETS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])
POPS = ("drop", "stand", "belly")
N, T = 8, 10
SEED = 5


def build_variant(tmp, k, dm, r):
    d = os.path.join(tmp, f"set{k}")
    os.makedirs(os.path.join(d, "oracle"))
    os.makedirs(os.path.join(d, "nightmare_rl_amd", "model"))
    for f in os.listdir(os.path.join(ROOT, "oracle")):
        if f.endswith(".c") or f == "nm_oracle.h":
            shutil.copy(os.path.join(ROOT, "oracle", f), os.path.join(d, "oracle", f))

    sys.path.insert(0, ROOT)
    from nightmare_rl_amd.model import compile_model as cm, payload as pl
    Tv = pl.modified_tables(dm, r)
    cm.emit_header(Tv, os.path.join(d, "nightmare_rl_amd", "model", "nm_model_data.h"))
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    cflags = re.search(r"^CFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()
    lib = os.path.join(d, "libnm_oracle.so")
    subprocess.check_call(["gcc"] + cflags + ["-shared", "-o", lib, "nm_oracle_physics.c", "nm_oracle_env.c", "-lm"], cwd=os.path.join(d, "oracle"))
    return lib, pl.row_of_tables(Tv)


def child(lib, out):
    """Runs in a process of its own: the oracle module bound to ONE variant library."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    orc.LIB_PATH = lib
    rng = np.random.default_rng(SEED)
    res = {}
    many = np.load(os.path.join(HERE, "env_manycontacts.npz"))["init_qpos"][:N]
    default = np.tile([0, np.pi / 5, 0], 6)
    for pop in POPS:
        o = orc.OracleEnv(N, seed=SEED)
        o.reset_idx()
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
        keys = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon")
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
            state()
        big = (np.stack(r["ncon"]) > 16).sum(axis=1)
        t0 = int(np.argmax([big[i:i + T].sum() for i in range(total - T + 1)]))
        for k in keys:
            res[f"{pop}_{k}"] = np.stack(r[k][t0:t0 + T + (len(r[k]) > total)])
    np.savez(out, **res)


def main():
    tmp = tempfile.mkdtemp(prefix="nm_payload_")
    try:
        parts = []
        rows = []
        for k, pay in enumerate(SETS):
            lib, row = build_variant(tmp, k, float(pay[0]), pay[1:])
            rows.append(row)
            out = os.path.join(tmp, f"set{k}.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, out])
            parts.append(np.load(out))
        g = {"sets": SETS, "rows": np.stack(rows)}
        for key in parts[0].files:
            g[key] = np.stack([p[key] for p in parts])          # [set, step (T or T + 1), env, ...]
        for pop in POPS:
            big = (g[f"{pop}_ncon"] > 16).sum(axis=(1, 2))
            con = (g[f"{pop}_ncon"] > 0).sum(axis=(1, 2))
            print(f"{pop}: env-steps with contacts per set {con.tolist()}, with more than 16 contacts {big.tolist()}, resets {g[f'{pop}_done'].sum(axis=(1, 2)).tolist()}")
        # base-body COM height of the standing robot: qpos z + (R ipos')_z
        q = g["stand_qpos"][:, 0]
        w, x, y, z = q[..., 3], q[..., 4], q[..., 5], q[..., 6]
        Rz = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], axis=-1)
        g["stand_height"] = (q[..., 2] + (Rz * g["rows"][:, None, 0:3]).sum(-1)).mean(axis=1)
        print("standing base height per set:", g["stand_height"].tolist())
        assert ((g["belly_ncon"] > 16).sum(axis=(1, 2)) >= 4).all(), "every set must exercise the matrix-free layout on several env-steps"
        np.savez_compressed(OUT, **g)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
        assert os.path.getsize(OUT) < (1 << 20)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
