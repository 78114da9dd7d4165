"""Generator of tests/golden/torque.npz: fp64 reference trajectories for the servo torque limit (nm_set_torque_limit), MuJoCo's actuator
forcerange.

Without a limit the oracle's servo force is unbounded: qfrc_actuator = kv clip(ctrl) - kv qvel, and every actuated dof enters the
implicit factor M + h kv I. Per env the oracle carries limits by joint type (oracle/nm_oracle.h: OracleEnv.set_torque_limit):
  * fwd_actuation: f = kv c - kv qvel becomes f > fmax ? fmax : (f < -fmax ? -fmax : f), fmax = limit[j % 3]            (mj_fwdActuation)
  * integrate: H[6+j][6+j] += h kv only where |qfrc_actuator[6+j]| < limit[j % 3]                    (mjd_actuator_vel in mj_implicit)
with a switch that turns the second off (the "force only" variant of condition e) and, per env, the smallest | |f| - fmax | seen over
finite limits, which this script reads after every step.

Sets (limits coxa / femur / tibia; kv) under SETS / KV; a mixed device batch gives env e set e % 5. Populations, seed, pre-rolls and action
streams are make_envparam_goldens.py's `drop` and `stand`; the pre-rolls run under the limits (in `stand` the robot settles under
its own limits). Per step: start state, inputs, obs, rew, done, ncon and the end-of-step qfrc_actuator.
Set 3 is (6.4, 0.3, 3.0): with a tibia limit of 2.4 (and 2.0 .. 2.8) some env of `drop` keeps its femur on the 0.3 bound for all 60
joint-steps, which condition b does not admit; at 3.0 every env leaves it at least once.

The script asserts, on the reference alone (the figures it prints are quoted in DESIGN 6.17):
  a  set 0 (infinite limits set) equals no limits set bit for bit: env_params.npz set 0, drop and stand;
  b  in drop every env of sets 1..4 has saturated and unsaturated joint-steps of every finitely limited joint type at the end of step
     (set 3's coxa limit of 6.4 is nearly unreachable and exempt);
  c  in stand, set 3 has all 60 femur joint-steps saturated in every env and no other joint saturated;
  d  every env of sets 1..3 departs from set 0 by more than 1e-5 in qpos;
  e  the variant with the clamp but without the factor mask departs from the full variant by more than 1e-4 in qpos in every env;
  f  the smallest saturation margin over the recorded window is above 1e-5 N m in every set and population;
  g  no done in any window.

    python tests/golden/make_torque_goldens.py            (CPU only, a few seconds)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_envparam_goldens as me      # noqa: E402  (the populations, seed, pre-rolls, action streams and the recorder)

OUT = os.path.join(HERE, "torque.npz")
INF = float("inf")
SETS = np.array([[INF, INF, INF], [3.2, 3.2, 3.2], [INF, 1.6, INF], [6.4, 0.3, 3.0], [2.0, 2.0, 2.0]])
KV = np.array([0.8, 0.8, 0.8, 0.8, 0.5])
POPS = ("drop", "stand")
N, T = me.N, me.T


def record(k, factor_mask):
    """All eight envs under set k."""
    def setup(o):
        o.set_torque_limit(SETS[k], factor_mask)
        o.set_env_params([me.SETS[0, 0], me.SETS[0, 1], KV[k]])

    def extra(o):
        return dict(qfrc=np.stack([o.data(i).np("qfrc_actuator")[6:].copy() for i in range(N)]), margin=np.float64(o.torque_limit()[1].min()))

    return me.record(setup, POPS, extra=extra)


def saturated(qfrc, limits):
    """[..., 18] bool: the joints whose recorded force sits on its bound."""
    return np.abs(qfrc) >= np.tile(limits, 6)


def main():
    full, force_only = [record(k, True) for k in range(len(SETS))], [record(k, False) for k in range(len(SETS))]
    g = {"sets": SETS, "kv": KV, **me.stacked(full)}
    ref = np.load(os.path.join(HERE, "env_params.npz"))
    for pop in POPS:
        for key in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "actions", "cmd_u", "obs", "rew", "done", "ncon"):      # a
            np.testing.assert_array_equal(g[f"{pop}_{key}"][0], ref[f"{pop}_{key}"][0], err_msg=f"{pop}_{key}")
    print("a: set 0 equals env_params.npz set 0 (no limits set) bit for bit, drop and stand")
    for pop in POPS:
        sat = np.stack([saturated(g[f"{pop}_qfrc"][k], SETS[k]) for k in range(len(SETS))])      # [set, T, N, 18]
        per_env = sat.sum(axis=(1, 3))
        moved = np.abs(g[f"{pop}_qpos"] - g[f"{pop}_qpos"][0]).max(axis=(1, 3))
        gap = np.stack([np.abs(full[k][f"{pop}_qpos"] - force_only[k][f"{pop}_qpos"]).max(axis=(0, 2)) for k in range(len(SETS))])
        margin = g[f"{pop}_margin"].min(axis=1)
        for k in range(len(SETS)):
            print(f"{pop} set {k}: saturated joint-steps of {T * 18} per env {per_env[k].tolist()}, max |qpos - set 0| per env "
                  f"{np.array2string(moved[k], precision=3)}, max |qpos - force-only variant| per env {np.array2string(gap[k], precision=3)}, "
                  f"smallest margin {margin[k]:.3g}, base z at the end {np.array2string(g[f'{pop}_qpos'][k, -1, :, 2], precision=3)}")
        assert per_env[0].sum() == 0
        if pop == "drop":      # b
            for k in range(1, len(SETS)):
                for jt in range(3):
                    if np.isfinite(SETS[k, jt]) and not (k == 3 and jt == 0):
                        n = sat[k][:, :, jt::3].sum(axis=(0, 2))
                        assert (n > 0).all() and (n < T * 6).all(), ("b", k, jt, n)
        else:      # c
            assert (sat[3][:, :, 1::3].sum(axis=(0, 2)) == T * 6).all() and sat[3][:, :, 0::3].sum() == 0 and sat[3][:, :, 2::3].sum() == 0, "c"
        assert (moved[1:4] > 1e-5).all(), "d"
        assert (gap[1:] > 1e-4).all(), "e"
        assert (margin[1:] > 1e-5).all(), ("f", margin)
        assert g[f"{pop}_done"].sum() == 0, "g"
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
