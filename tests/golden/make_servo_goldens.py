"""Generator of tests/golden/servo.npz: fp64 reference trajectories for the servo target model (nm_set_servo), alone and behind
per-env actuation latency.

The oracle commands every servo with ((a_t - default) - dof_pos) p_gain. The variant recorded here is the oracle source with the two
places of nmo_env_step that make_latency_goldens.py patches - the line that turns the step's action into the servo command, and the call
that runs the step's DECIMATION substeps - patched in a temporary copy (oracle/ itself is not touched), with latency and the servo model
in ONE patch set. The delay line is make_latency_goldens.py's. Behind it, per env, sit a row (rate, d_gain) and the limited targets
L[18]: with T = (double)a - default the target of the late action a_{t-k},
    d = T - L;   L' = |d| <= rate ? T : L + copysign(rate, d)
    ctrl = (L_used - dof_pos) P_GAIN - d_gain dof_vel        (dof_pos, dof_vel: the step-start buffers)
where the r substeps before the switch use L and the rest L'. Everything else of the step is the oracle's, so it keeps a_t.

Populations, seed and pre-roll are the latency fixture's (drop: 7 steps, stand: 150). The pre-roll runs with the servo model off; where
the recorded window starts the model is switched on with L = the target of the last late action, a_{t-1-k} - default: what a servo
without a limit holds there. Two recordings under ROWS: S (latency off) and SL (the delays of latency.npz). Every step's start state is
recorded with L and the history.

The script asserts, on the reference alone:
  * default rows (inf, 0), latency off: the patched library equals the unpatched one bit for bit;
  * default rows under the delays: it equals tests/golden/latency.npz bit for bit;
  * in both populations and both recordings every env with a non-default row departs from its nominal run (default rows) by more than
    1e-5 in qpos, and env 0 by nothing;
  * every env with a finite rate has at least one saturated and one unsaturated joint-step in the recorded window - in `stand` this is
    required of the envs with rate <= 0.04 only (its small actions never move a target by 0.08 in one step).

    python tests/golden/make_servo_goldens.py            (CPU only, about a minute)
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_latency_goldens as lat      # noqa: E402  (the delay line's patch, the populations, the seed and the library recipe)

OUT = os.path.join(HERE, "servo.npz")
INF = float("inf")
RATE = np.array([INF, 0.03, 0.02, 0.08, 0.04, INF, 0.02, 0.08])      # the two envs of a wave always differ
D_GAIN = np.array([0.0, 0.0, 0.05, 0.05, 0.2, 0.2, 0.0, 0.1])      # env 0 default; 1 and 6 the limiter only; 5 d_gain only
ROWS = np.stack([RATE, D_GAIN], axis=1)
DEFAULT_ROWS = np.tile([INF, 0.0], (8, 1))
DELAYS, POPS, N, T, H, SEED = lat.DELAYS, lat.POPS, lat.N, lat.T, lat.H, lat.SEED
DECIMATION = 2
DEFAULT_POS = np.tile([0.0, np.pi / 5, 0.0], 6)

STATE = lat.STATE.replace("\nvoid nmo_env_step(nmo_env* e,", """
/* ---- servo target model (tests/golden/make_servo_goldens.py) */
static double* g_srv_rows = NULL; /* [N][2] (rate, d_gain), NULL = off */
static double* g_srv_lim = NULL;  /* [N][18] limited targets */
void nmo_servo_set(int N, const double* rows, const double* lim) {
  free(g_srv_rows); free(g_srv_lim);
  g_srv_rows = NULL; g_srv_lim = NULL;
  if (!rows) return;
  g_srv_rows = (double*)malloc(sizeof(double) * N * 2);
  memcpy(g_srv_rows, rows, sizeof(double) * N * 2);
  g_srv_lim = (double*)malloc(sizeof(double) * N * 18);
  memcpy(g_srv_lim, lim, sizeof(double) * N * 18);
}
double* nmo_servo_lim(void) { return g_srv_lim; }

void nmo_env_step(nmo_env* e,""")
assert STATE != lat.STATE

SERVO_CTRL = """        if (g_srv_rows) {      /* the limiter sits behind the delay line: it runs on the late action's target */
          const double t_ = (double)al_ - default_pos[j % 3], l_ = g_srv_lim[i * 18 + j], dd_ = t_ - l_;
          const double rate_ = g_srv_rows[i * 2], dg_ = g_srv_rows[i * 2 + 1];
          const double ln_ = fabs(dd_) <= rate_ ? t_ : l_ + copysign(rate_, dd_);
          e->data[i].ctrl[j] = ((r_ > 0 ? l_ : ln_) - e->dof_pos[i * 18 + j]) * P_GAIN - dg_ * e->dof_vel[i * 18 + j];
          g_lat_late[i * 18 + j] = (ln_ - e->dof_pos[i * 18 + j]) * P_GAIN - dg_ * e->dof_vel[i * 18 + j];
          g_srv_lim[i * 18 + j] = ln_;
        }
      }
"""
assert lat.CTRL_NEW.endswith("      }\n")
CTRL_NEW = lat.CTRL_NEW[:-len("      }\n")] + SERVO_CTRL


def build_variant(tmp, name, patched):
    """make_latency_goldens.build_variant with this file's patch set."""
    saved = lat.STATE, lat.CTRL_NEW
    lat.STATE, lat.CTRL_NEW = STATE, CTRL_NEW
    try:
        return lat.build_variant(tmp, name, patched)
    finally:
        lat.STATE, lat.CTRL_NEW = saved


MODES = {      # name: (library, delays or None = no delay line at all, servo rows or None)
    "plain": ("plain", None, None),
    "zero": ("patched", np.zeros(N, np.int32), DEFAULT_ROWS),
    "delays": ("patched", DELAYS, DEFAULT_ROWS),
    "S": ("patched", np.zeros(N, np.int32), ROWS),
    "SL": ("patched", DELAYS, ROWS),
}


def child(lib, out, mode):
    """Runs in a process of its own: the oracle module bound to ONE library."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    orc.LIB_PATH = lib
    L = orc.lib()
    _, delays, rows = MODES[mode]
    if mode != "plain":
        L.nmo_lat_set.argtypes = [C.c_int, C.c_void_p]
        L.nmo_lat_hist.restype = C.POINTER(C.c_float)
        L.nmo_servo_set.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.nmo_servo_lim.restype = C.POINTER(C.c_double)
    rng = np.random.default_rng(SEED)
    res = {}
    for pop in POPS:
        o = orc.OracleEnv(N, seed=SEED)
        if mode != "plain":
            L.nmo_servo_set(N, None, None)
            L.nmo_lat_set(N, delays.ctypes.data_as(C.c_void_p))        # a fresh, zero history
        o.reset_idx()
        if pop == "drop":
            pre, act = 7, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        else:
            pre, act = 150, lambda: rng.uniform(-0.12, 0.12, (N, 18)).astype(np.float32)
        past = []      # the scaled and clipped actions of the pre-roll, the oracle's own buffer after each step
        for _ in range(pre):
            o.step(act())
            past.append(o.get_buffers()["actions"].copy())
        if mode != "plain":      # the servo model comes on here, holding the target of the last late action a_{t-1-k}
            k = delays // DECIMATION
            lim0 = np.stack([past[-1 - k[e]][e] - DEFAULT_POS for e in range(N)])
            r64 = np.ascontiguousarray(rows, np.float64)
            L.nmo_servo_set(N, r64.ctypes.data_as(C.c_void_p), np.ascontiguousarray(lim0).ctypes.data_as(C.c_void_p))
        keys = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "hist", "lim", "actions", "cmd_u", "obs", "rew", "done", "ncon")
        r = {k_: [] for k_ in keys}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"])
            if mode != "plain":
                r["hist"].append(np.ctypeslib.as_array(L.nmo_lat_hist(), (N, H, 18)).copy())
                r["lim"].append(np.ctypeslib.as_array(L.nmo_servo_lim(), (N, 18)).copy())
            else:
                r["hist"].append(np.zeros((N, H, 18), np.float32))
                r["lim"].append(np.zeros((N, 18)))

        state()
        for t in range(T):
            a = act()
            cu = rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            state()
        for k_ in keys:
            res[f"{pop}_{k_}"] = np.stack(r[k_])
    np.savez(out, **res)


def saturation(g, pop, delays):
    """[T, N, 18] bool: the joint-steps of a recording whose limiter saturated, L' != T, from the recorded L, history and actions."""
    k = delays // DECIMATION
    sat = np.zeros((T, N, 18), bool)
    for t in range(T):
        for e in range(N):
            a = g[f"{pop}_act"][t + 1][e] if k[e] == 0 else g[f"{pop}_hist"][t][e, k[e] - 1].astype(np.float64)
            sat[t, e] = g[f"{pop}_lim"][t + 1][e] != a - DEFAULT_POS
    return sat


def main():
    tmp = tempfile.mkdtemp(prefix="nm_servo_")
    try:
        libs = {"plain": build_variant(tmp, "plain", False), "patched": build_variant(tmp, "patched", True)}
        outs = {}
        for mode, (lib, _, _) in MODES.items():
            out = os.path.join(tmp, f"{mode}.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", libs[lib], out, mode])
            outs[mode] = dict(np.load(out))
        for key in outs["plain"]:        # default rows change nothing
            if not key.endswith(("_hist", "_lim")):
                np.testing.assert_array_equal(outs["plain"][key], outs["zero"][key], err_msg=key)
        print("patched oracle with default servo rows, latency off, equals the unpatched oracle bit for bit")
        latency = np.load(os.path.join(HERE, "latency.npz"))
        for key in latency.files:
            if key != "delays":
                np.testing.assert_array_equal(latency[key], outs["delays"][key], err_msg=key)
        print("patched oracle with default servo rows under the delays equals latency.npz bit for bit")
        g = {"rate": RATE, "d_gain": D_GAIN, "delays": DELAYS}
        changed = (RATE != INF) | (D_GAIN != 0)
        for rec, nominal, delays in (("S", "zero", np.zeros(N, np.int32)), ("SL", "delays", DELAYS)):
            o = outs[rec]
            for pop in POPS:
                moved = np.abs(o[f"{pop}_qpos"] - outs[nominal][f"{pop}_qpos"]).max(axis=(0, 2))
                sat = saturation(o, pop, delays).sum(axis=(0, 2))
                print(f"{rec} {pop}: env-steps with contacts {(o[f'{pop}_ncon'] > 0).sum()} of {N * T}, resets {int(o[f'{pop}_done'].sum())}, "
                      f"max |qpos - nominal qpos| per env {np.array2string(moved, precision=2)}, saturated joint-steps of {T * 18} per env {sat}")
                assert (moved[changed] > 1e-5).all() and (moved[~changed] == 0).all(), "an env with a non-default row must depart from its nominal run, env 0 must not"
                need = np.isfinite(RATE) & ((RATE <= 0.04) | (pop == "drop"))
                assert (sat[need] > 0).all() and (sat[need] < T * 18).all(), "a finite rate must show both branches of the limiter"
                assert (sat[~np.isfinite(RATE)] == 0).all()
                np.testing.assert_array_equal(o[f"{pop}_hist"][1:, :, 0], o[f"{pop}_act"][1:].astype(np.float32))
            for key, val in o.items():
                g[f"{rec}_{key}"] = val
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
