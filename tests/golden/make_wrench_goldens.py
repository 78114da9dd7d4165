"""Generator of tests/golden/wrench.npz: fp64 reference trajectories for the external wrench on the base (nm_set_base_wrench), MuJoCo's
xfrc_applied on the base body.

The oracle applies no external force: fwd_acceleration forms qfrc_smooth = -qfrc_bias + qfrc_actuator. The variant recorded here is the
oracle source with that line of nm_oracle_physics.c patched in a temporary copy (the recipe of make_torque_goldens.py; oracle/ itself is
not touched), the patch asserted to apply exactly once: behind the line, qfrc_smooth += J'[F; tau] with the translational Jacobian of
the point xipos[base] taken from the oracle's OWN jac_point (mj_jac over cdof, about the subtree COM) and the rotational Jacobian read
from cdof's rotational half. The device kernel uses the closed form of the free joint instead (qfrc[0:3] += F, qfrc[3:6] += Rb' tau +
ipos x Rb' F): two routes, and this fixture is where they have to agree - in particular on the frame of the three rotational dofs.
The wrench is process-wide (one uniform set per child process, one OpenMP thread).

Sets (F in N, tau in N m, world frame) under SETS; set 3 also carries a payload with a displaced COM (PAYLOAD: its library is compiled
against the header compile_model.emit_header writes for payload.modified_tables, make_payload_goldens.py's recipe), so that the base's
ipos differs from the model's. A mixed device batch gives env e set e % 5. Populations, seed, pre-rolls and action streams are
make_envparam_goldens.py's `drop` and `stand`; the pre-rolls run in the variant itself (the wrench acts from the first step). Per step:
start state, inputs, obs, rew, done, ncon.

The script asserts, on the reference alone (the figures it prints are quoted in DESIGN 6.19):
  a  set 0 equals the unpatched oracle bit for bit: env_params.npz set 0, drop and stand;
  b  every env of sets 1..4 departs from set 0 by more than 1e-5 in qpos (set 3: from its own payload under a zero wrench as well);
  c  pure tau (set 2) and pure F (set 1) depart from each other by more than 1e-5 in qpos in every env;
  d  no done in any window.

    python tests/golden/make_wrench_goldens.py            (CPU only, about a minute)
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
OUT = os.path.join(HERE, "wrench.npz")
# (Fx, Fy, Fz, tx, ty, tz)
SETS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                 [3.0, -2.0, 4.0, 0.0, 0.0, 0.0],
                 [0.0, 0.0, 0.0, 0.3, -0.2, 0.25],
                 [-2.0, 3.0, 2.0, 0.2, 0.3, -0.3],
                 [4.0, 1.0, -3.0, -0.25, 0.15, 0.2]])
# (dm kg, r m) per set: set 3 carries make_payload_goldens.py's camera mast, whose COM is displaced on all three axes
PAYLOAD = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05], [0.0, 0.0, 0.0, 0.0]])
POPS = ("drop", "stand")
N, T = 8, 10
SEED = 5

LINE_OLD = "  for (int i = 0; i < NV; i++) d->qfrc_smooth[i] = -d->qfrc_bias[i] + d->qfrc_actuator[i]; /* passive, applied = 0 */"
LINE_NEW = LINE_OLD.replace("/* passive, applied = 0 */", "/* passive = 0 */") + """
  { /* xfrc_applied on the base body (tests/golden/make_wrench_goldens.py): J'[F; tau], F at xipos, through mj_jac's own route */
    double jp_[3][NV];
    jac_point(d, jp_, 1, d->xipos[1]);
    for (int i = 0; i < 6; i++) {
      double s_ = 0;
      for (int k = 0; k < 3; k++) s_ += jp_[k][i] * g_wrench[k] + d->cdof[i][k] * g_wrench[3 + k];
      d->qfrc_smooth[i] += s_;
    }
  }"""
HEAD_OLD = "static void fwd_acceleration(nmo_data* d) {"
HEAD_NEW = """/* ---- external wrench on the base (tests/golden/make_wrench_goldens.py) */
static double g_wrench[6] = {0, 0, 0, 0, 0, 0};
void nmo_wrench_set(const double* w) { for (int k = 0; k < 6; k++) g_wrench[k] = w[k]; }
static void fwd_acceleration(nmo_data* d) {"""


def build_variant(tmp, name, payload, patched=True):
    d = os.path.join(tmp, name)
    os.makedirs(os.path.join(d, "oracle"))
    os.makedirs(os.path.join(d, "nightmare_rl_amd", "model"))
    for f in os.listdir(os.path.join(ROOT, "oracle")):
        if f.endswith(".c") or f == "nm_oracle.h":
            shutil.copy(os.path.join(ROOT, "oracle", f), os.path.join(d, "oracle", f))
    hdr = os.path.join(d, "nightmare_rl_amd", "model", "nm_model_data.h")
    row = None
    if payload[0] != 0.0:
        sys.path.insert(0, ROOT)
        from nightmare_rl_amd.model import compile_model as cm, payload as pl
        Tv = pl.modified_tables(float(payload[0]), payload[1:])
        cm.emit_header(Tv, hdr)
        row = pl.row_of_tables(Tv)
    else:
        shutil.copy(os.path.join(ROOT, "nightmare_rl_amd", "model", "nm_model_data.h"), hdr)
    if patched:
        phys = os.path.join(d, "oracle", "nm_oracle_physics.c")
        s = open(phys).read()
        for old, new in ((HEAD_OLD, HEAD_NEW), (LINE_OLD, LINE_NEW)):
            assert s.count(old) == 1, old
            s = s.replace(old, new)
        open(phys, "w").write(s)
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    cflags = re.search(r"^CFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()
    lib = os.path.join(d, "libnm_oracle.so")
    subprocess.check_call(["gcc"] + cflags + ["-shared", "-o", lib, "nm_oracle_physics.c", "nm_oracle_env.c", "-lm"], cwd=os.path.join(d, "oracle"))
    return lib, row


def child(lib, out, wrench):
    """Runs in a process of its own: the oracle module bound to ONE variant library, under one wrench."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    orc.LIB_PATH = lib
    L = orc.lib()
    L.nmo_wrench_set.argtypes = [C.c_void_p]
    w = np.ascontiguousarray(wrench, np.float64)
    rng = np.random.default_rng(SEED)
    res = {}
    for pop in POPS:
        o = orc.OracleEnv(N, seed=SEED)
        o.reset_idx()
        L.nmo_wrench_set(w.ctypes.data_as(C.c_void_p))
        if pop == "drop":
            pre, act = 7, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        else:
            pre, act = 150, lambda: np.zeros((N, 18), np.float32)
        for _ in range(pre):
            o.step(act())
        keys = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon")
        r = {k_: [] for k_ in keys}

        def state():
            q, v, qw = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(qw); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"])

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


def main():
    tmp = tempfile.mkdtemp(prefix="nm_wrench_")
    env = dict(os.environ, OMP_NUM_THREADS="1")

    def run(lib, name, wrench):
        out = os.path.join(tmp, name + ".npz")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, out] + [repr(float(x)) for x in wrench], env=env)
        return dict(np.load(out))

    try:
        parts, rows = [], []
        for k in range(len(SETS)):
            lib, row = build_variant(tmp, f"set{k}", PAYLOAD[k])
            parts.append(run(lib, f"set{k}", SETS[k]))
            if row is not None:
                rows.append(row)
                bare = run(lib, f"set{k}_bare", np.zeros(6))      # the same payload under a zero wrench
        g = {"sets": SETS, "payload": PAYLOAD, "payload_row": np.stack(rows)}
        for key in parts[0]:
            g[key] = np.stack([p[key] for p in parts])          # [set, step (T or T + 1), env, ...]
        ref = np.load(os.path.join(HERE, "env_params.npz"))
        for pop in POPS:
            for key in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon"):      # a
                np.testing.assert_array_equal(g[f"{pop}_{key}"][0], ref[f"{pop}_{key}"][0], err_msg=f"{pop}_{key}")
        print("a: set 0 equals env_params.npz set 0 (the unpatched oracle) bit for bit, drop and stand")
        for pop in POPS:
            q = g[f"{pop}_qpos"]
            moved = np.abs(q - q[0]).max(axis=(1, 3))
            own = np.abs(q[3] - bare[f"{pop}_qpos"]).max(axis=(0, 2))
            apart = np.abs(q[1] - q[2]).max(axis=(0, 2))
            for k in range(len(SETS)):
                print(f"{pop} set {k}: max |qpos - set 0| per env {np.array2string(moved[k], precision=3)}, base z at the end "
                      f"{np.array2string(q[k, -1, :, 2], precision=3)}, env-steps with contacts {(g[f'{pop}_ncon'][k] > 0).sum()}")
            print(f"{pop}: set 3 against its payload under a zero wrench, max |dqpos| per env {np.array2string(own, precision=3)}; "
                  f"pure F against pure tau {np.array2string(apart, precision=3)}")
            assert (moved[1:] > 1e-5).all() and (own > 1e-5).all(), "b"
            assert (apart > 1e-5).all(), "c"
            assert g[f"{pop}_done"].sum() == 0, "d"
        np.savez_compressed(OUT, **g)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
        assert os.path.getsize(OUT) < (1 << 20)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) == 10 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], [float(x) for x in sys.argv[4:]])
    else:
        main()
