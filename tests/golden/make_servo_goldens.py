"""Generator of tests/golden/servo.npz: fp64 reference trajectories for the servo target model (nm_set_servo), alone and behind
per-env actuation latency.

Without the model the oracle commands every servo with ((a_t - default) - dof_pos) p_gain. The model (oracle/nm_oracle.h:
OracleEnv.set_servo) sits behind make_latency_goldens.py's delay line: per env a row (rate, d_gain) and the limited targets L[18]; with
T = (double)a - default the target of the late action a_{t-k},
    d = T - L;   L' = |d| <= rate ? T : L + copysign(rate, d)
    ctrl = (L_used - dof_pos) P_GAIN - d_gain dof_vel        (dof_pos, dof_vel: the step-start buffers)
where the r substeps before the switch use L and the rest L'. Everything else of the step keeps a_t.

Populations, seed and pre-roll are the latency fixture's (drop: 7 steps, stand: 150). The pre-roll runs under the default row (inf, 0);
where the recorded window starts the rows are set, and L is the target of the last late action, a_{t-1-k} - default: what a servo
without a limit holds there (asserted against the oracle's own L, which follows the late target under the default row). Two recordings
under ROWS: S (latency off) and SL (the delays of latency.npz). Every step's start state is recorded with L and the history.

The script asserts, on the reference alone:
  * default rows (inf, 0) set, latency off: equal to no rows set at all bit for bit;
  * default rows set under the delays: equal to tests/golden/latency.npz bit for bit;
  * in both populations and both recordings every env with a non-default row departs from its nominal run (default rows) by more than
    1e-5 in qpos, and env 0 by nothing;
  * every env with a finite rate has at least one saturated and one unsaturated joint-step in the recorded window - in `stand` this is
    required of the envs with rate <= 0.04 only (its small actions never move a target by 0.08 in one step).

    python tests/golden/make_servo_goldens.py            (CPU only, a few seconds)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_latency_goldens as lat      # noqa: E402  (the populations, the seed and the recorder)

OUT = os.path.join(HERE, "servo.npz")
INF = float("inf")
RATE = np.array([INF, 0.03, 0.02, 0.08, 0.04, INF, 0.02, 0.08])      # the two envs of a wave always differ
D_GAIN = np.array([0.0, 0.0, 0.05, 0.05, 0.2, 0.2, 0.0, 0.1])      # env 0 default; 1 and 6 the limiter only; 5 d_gain only
ROWS = np.stack([RATE, D_GAIN], axis=1)
DEFAULT_ROWS = np.tile([INF, 0.0], (8, 1))
DELAYS, POPS, N, T, H, SEED = lat.DELAYS, lat.POPS, lat.N, lat.T, lat.H, lat.SEED
DECIMATION = 2
DEFAULT_POS = np.tile([0.0, np.pi / 5, 0.0], 6)

MODES = {      # name: (delays or None = never set, servo rows or None = never set)
    "plain": (None, None),
    "zero": (np.zeros(N, np.int32), DEFAULT_ROWS),
    "delays": (DELAYS, DEFAULT_ROWS),
    "S": (np.zeros(N, np.int32), ROWS),
    "SL": (DELAYS, ROWS),
}


def record(mode):
    delays, rows = MODES[mode]

    def window(o, past):      # the servo rows come on here; L holds the target of the last late action a_{t-1-k}
        k = (np.zeros(N, np.int32) if delays is None else delays) // DECIMATION
        np.testing.assert_array_equal(o.servo_state()[1], np.stack([past[-1 - k[e]][e] - DEFAULT_POS for e in range(N)]))
        if rows is not None:
            o.set_servo(rows)

    return lat.record(delays, window, extra_keys=("lim",))


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
    outs = {mode: record(mode) for mode in MODES}
    for key in outs["plain"]:        # default rows change nothing
        np.testing.assert_array_equal(outs["plain"][key], outs["zero"][key], err_msg=key)
    print("default servo rows, latency off, equal no rows set bit for bit")
    latency = np.load(os.path.join(HERE, "latency.npz"))
    for key in latency.files:
        if key != "delays":
            np.testing.assert_array_equal(latency[key], outs["delays"][key], err_msg=key)
    print("default servo rows under the delays equal latency.npz bit for bit")
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


if __name__ == "__main__":
    main()
