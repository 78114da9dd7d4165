"""Generator of tests/golden/latency.npz: fp64 reference trajectories for per-env actuation latency (nm_set_action_latency).

The oracle applies every action in the step it was given. A DELAYED variant is the oracle source with two places of nmo_env_step patched
in a temporary copy (oracle/ itself is not touched): the line that turns the step's action into the servo command, and the call that
runs the step's DECIMATION physics substeps. The patched copy keeps, per env, a delay d in substeps and the last H = 3 scaled and
clipped float actions (hist[j] = a_{t-1-j}); with k = d / DECIMATION, r = d % DECIMATION it runs r substeps under the command of
a_{t-k-1}, then DECIMATION - r under that of a_{t-k} (a_t itself where k = 0), each command being the oracle's own expression on the same
dof_pos snapshot; then it shifts the history. Everything else of the step (observation, rewards, action buffers) is the oracle's, so it
keeps a_t.

The script first asserts that the patched library at delay 0 equals the unpatched one bit for bit over both populations, then records,
free-running (every step's start state is the previous step's end state), with the delays DELAYS over the eight envs:
    drop   random actions while the robot falls from the initial pose and lands
    stand  small random actions, new every step, after the robot has settled on its feet under such actions
Both libraries are built with the flags of oracle/Makefile and driven through oracle/oracle.py in child processes (one library per
process). Nothing but the .npz is written into the tree.

    python tests/golden/make_latency_goldens.py            (CPU only, well under a minute)
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "latency.npz")
DELAYS = np.array([0, 1, 2, 3, 4, 5, 6, 0], np.int32)      # a two-env wave (2w, 2w + 1) always holds two different switch substeps r
POPS = ("drop", "stand")
N, T, H = 8, 10, 3
SEED = 5

STATE = """
/* ---- actuation latency (tests/golden/make_latency_goldens.py): one env object per process */
static int* g_lat_delay = NULL;   /* [N] substeps, NULL = off */
static float* g_lat_hist = NULL;  /* [N][3][18], hist[j] = a_{t-1-j} */
static double* g_lat_late = NULL; /* [N][18] the command the env switches to at substep r */
void nmo_lat_set(int N, const int* delay) {
  free(g_lat_delay); free(g_lat_hist); free(g_lat_late);
  g_lat_delay = NULL; g_lat_hist = NULL; g_lat_late = NULL;
  if (!delay) return;
  g_lat_delay = (int*)malloc(sizeof(int) * N);
  memcpy(g_lat_delay, delay, sizeof(int) * N);
  g_lat_hist = (float*)calloc((size_t)N * 54, sizeof(float));
  g_lat_late = (double*)calloc((size_t)N * 18, sizeof(double));
}
float* nmo_lat_hist(void) { return g_lat_hist; }

void nmo_env_step(nmo_env* e,"""

CTRL_OLD = "      e->data[i].ctrl[j] = (((double)e->actions[i * 18 + j] - default_pos[j % 3]) - e->dof_pos[i * 18 + j]) * P_GAIN;\n"
CTRL_NEW = """      {
        const int d_ = g_lat_delay ? g_lat_delay[i] : 0, k_ = d_ / DECIMATION, r_ = d_ % DECIMATION;
        const float* hi_ = g_lat_hist ? g_lat_hist + i * 54 : NULL;
        const float al_ = k_ == 0 ? e->actions[i * 18 + j] : hi_[(k_ - 1) * 18 + j];   /* a_{t-k}: substeps s >= r */
        const float ae_ = r_ > 0 ? hi_[k_ * 18 + j] : al_;                              /* a_{t-k-1}: substeps s < r */
        e->data[i].ctrl[j] = (((double)ae_ - default_pos[j % 3]) - e->dof_pos[i * 18 + j]) * P_GAIN;
        if (g_lat_late) g_lat_late[i * 18 + j] = (((double)al_ - default_pos[j % 3]) - e->dof_pos[i * 18 + j]) * P_GAIN;
      }
"""
STEP_OLD = "    nmo_step(&e->data[i], s, DECIMATION);\n  }\n  /* E3 (env.py:212-232) */"
STEP_NEW = """    {
      const int r_ = g_lat_delay ? g_lat_delay[i] % DECIMATION : 0;
      if (r_ > 0) {
        nmo_step(&e->data[i], s, r_);
        for (int j = 0; j < 18; j++) e->data[i].ctrl[j] = g_lat_late[i * 18 + j];
        nmo_step(&e->data[i], s, DECIMATION - r_);
      } else nmo_step(&e->data[i], s, DECIMATION);
      if (g_lat_hist) {
        float* hi_ = g_lat_hist + i * 54;
        memmove(hi_ + 18, hi_, sizeof(float) * 36);
        memcpy(hi_, e->actions + i * 18, sizeof(float) * 18);
      }
    }
  }
  /* E3 (env.py:212-232) */"""


def build_variant(tmp, name, patched):
    d = os.path.join(tmp, name)
    os.makedirs(os.path.join(d, "oracle"))
    os.makedirs(os.path.join(d, "nightmare_rl_amd", "model"))
    for f in os.listdir(os.path.join(ROOT, "oracle")):
        if f.endswith(".c") or f == "nm_oracle.h":
            shutil.copy(os.path.join(ROOT, "oracle", f), os.path.join(d, "oracle", f))
    shutil.copy(os.path.join(ROOT, "nightmare_rl_amd", "model", "nm_model_data.h"), os.path.join(d, "nightmare_rl_amd", "model", "nm_model_data.h"))
    if patched:
        path = os.path.join(d, "oracle", "nm_oracle_env.c")
        s = open(path).read()
        for old, new in (("\nvoid nmo_env_step(nmo_env* e,", STATE), (CTRL_OLD, CTRL_NEW), (STEP_OLD, STEP_NEW)):
            assert s.count(old) == 1, old
            s = s.replace(old, new)
        open(path, "w").write(s)
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    cflags = re.search(r"^CFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()
    lib = os.path.join(d, "libnm_oracle.so")
    subprocess.check_call(["gcc"] + cflags + ["-shared", "-o", lib, "nm_oracle_physics.c", "nm_oracle_env.c", "-lm"], cwd=os.path.join(d, "oracle"))
    return lib


def child(lib, out, mode):
    """Runs in a process of its own: the oracle module bound to ONE library. mode: "plain" (the unpatched library), "zero" (patched, delay 0
    in every env), "delays" (patched, DELAYS)."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    orc.LIB_PATH = lib
    L = orc.lib()
    if mode != "plain":
        L.nmo_lat_set.argtypes = [C.c_int, C.c_void_p]
        L.nmo_lat_hist.restype = C.POINTER(C.c_float)
    delays = DELAYS if mode == "delays" else np.zeros(N, np.int32)
    rng = np.random.default_rng(SEED)
    res = {}
    for pop in POPS:
        o = orc.OracleEnv(N, seed=SEED)
        if mode != "plain":
            L.nmo_lat_set(N, delays.ctypes.data_as(C.c_void_p))        # a fresh, zero history
        o.reset_idx()
        if pop == "drop":
            pre, act = 7, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        else:
            pre, act = 150, lambda: rng.uniform(-0.12, 0.12, (N, 18)).astype(np.float32)
        for _ in range(pre):
            o.step(act())
        keys = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "hist", "actions", "cmd_u", "obs", "rew", "done", "ncon")
        r = {k: [] for k in keys}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"])
            if mode != "plain":
                r["hist"].append(np.ctypeslib.as_array(L.nmo_lat_hist(), (N, H, 18)).copy())
            else:
                r["hist"].append(np.zeros((N, H, 18), np.float32))

        state()
        for t in range(T):
            a = act()
            cu = rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            state()
        for k in keys:
            res[f"{pop}_{k}"] = np.stack(r[k])
    np.savez(out, **res)


def main():
    tmp = tempfile.mkdtemp(prefix="nm_latency_")
    try:
        plain, patched = build_variant(tmp, "plain", False), build_variant(tmp, "patched", True)
        outs = {}
        for mode, lib in (("plain", plain), ("zero", patched), ("delays", patched)):
            out = os.path.join(tmp, f"{mode}.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, out, mode])
            outs[mode] = dict(np.load(out))
        for key in outs["plain"]:        # the patch changes nothing at delay 0
            if not key.endswith("_hist"):
                np.testing.assert_array_equal(outs["plain"][key], outs["zero"][key], err_msg=key)
        print("patched oracle at delay 0 equals the unpatched oracle bit for bit")
        g = outs["delays"]
        g["delays"] = DELAYS
        for pop in POPS:
            moved = np.abs(g[f"{pop}_qpos"] - outs["zero"][f"{pop}_qpos"]).max(axis=(0, 2))
            print(f"{pop}: env-steps with contacts {(g[f'{pop}_ncon'] > 0).sum()} of {N * T}, resets {int(g[f'{pop}_done'].sum())}, "
                  f"max |qpos - undelayed qpos| per env {np.array2string(moved, precision=2)}")
            assert (moved[DELAYS > 0] > 1e-6).all() and (moved[DELAYS == 0] == 0).all(), "a delayed env must differ from its undelayed run, an undelayed one must not"
            # the recorded histories are the recorded actions, scaled and clipped by the oracle (its actions buffer)
            np.testing.assert_array_equal(g[f"{pop}_hist"][1:, :, 0], g[f"{pop}_act"][1:].astype(np.float32))
        np.savez_compressed(OUT, **g)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
        assert os.path.getsize(OUT) < (1 << 20)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main()
