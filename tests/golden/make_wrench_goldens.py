"""Generator of tests/golden/wrench.npz: fp64 reference trajectories for the external wrench on the base (nm_set_base_wrench), MuJoCo's
xfrc_applied on the base body.

Without a wrench fwd_acceleration forms qfrc_smooth = -qfrc_bias + qfrc_actuator. Per env the oracle carries a wrench [F; tau]
(oracle/nm_oracle.h: OracleEnv.set_base_wrench): behind that line, qfrc_smooth += J'[F; tau] with the translational Jacobian of the
point xipos[base] taken from the oracle's OWN jac_point (mj_jac over cdof, about the subtree COM) and the rotational Jacobian read from
cdof's rotational half. The device kernel uses the closed form of the free joint instead (qfrc[0:3] += F, qfrc[3:6] += Rb' tau +
ipos x Rb' F): two routes, and this fixture is where they have to agree - in particular on the frame of the three rotational dofs.

Sets (F in N, tau in N m, world frame) under SETS; set 3 also carries a payload with a displaced COM (PAYLOAD: its library is compiled
against the header of the recompiled model, make_payload_goldens.payload_lib - the one library this script builds), so that the base's
ipos differs from the model's. A mixed device batch gives env e set e % 5. Populations, seed, pre-rolls and action streams are
make_envparam_goldens.py's `drop` and `stand`; the pre-rolls run under the wrench (it acts from the first step). Per step:
start state, inputs, obs, rew, done, ncon.

The script asserts, on the reference alone (the figures it prints are quoted in DESIGN 6.19):
  a  set 0 (a zero wrench set) equals no wrench set bit for bit: env_params.npz set 0, drop and stand;
  b  every env of sets 1..4 departs from set 0 by more than 1e-5 in qpos (set 3: from its own payload under a zero wrench as well);
  c  pure tau (set 2) and pure F (set 1) depart from each other by more than 1e-5 in qpos in every env;
  d  no done in any window.

    python tests/golden/make_wrench_goldens.py            (CPU only, a few seconds)
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_payload_goldens as mp      # noqa: E402  (payload_lib)
import make_envparam_goldens as me      # noqa: E402  (the populations, seed, pre-rolls, action streams and the recorder)

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
N, T = me.N, me.T


def main():
    tmp = tempfile.mkdtemp(prefix="nm_wrench_")
    try:
        parts, rows = [], []
        for k in range(len(SETS)):
            lib = None
            if PAYLOAD[k, 0] != 0.0:
                lib, row = mp.payload_lib(tmp, PAYLOAD[k, 0], PAYLOAD[k, 1:])
                rows.append(row)
                bare = me.record(lambda o: o.set_base_wrench(np.zeros(6)), POPS, lib)      # the same payload under a zero wrench
            parts.append(me.record(lambda o, k=k: o.set_base_wrench(SETS[k]), POPS, lib))
        g = {"sets": SETS, "payload": PAYLOAD, "payload_row": np.stack(rows), **me.stacked(parts)}
        ref = np.load(os.path.join(HERE, "env_params.npz"))
        for pop in POPS:
            for key in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon"):      # a
                np.testing.assert_array_equal(g[f"{pop}_{key}"][0], ref[f"{pop}_{key}"][0], err_msg=f"{pop}_{key}")
        print("a: set 0 equals env_params.npz set 0 (no wrench set) bit for bit, drop and stand")
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
    main()
