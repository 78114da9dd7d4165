"""Generator of tests/golden/gravity.npz: fp64 reference trajectories for per-env gravity vectors (slopes and gravity offsets).

For an infinite plane a floor inclined by theta is a level floor under a gravity vector tilted by theta, written in the floor's frame. The
oracle carries two vectors per env (oracle/nm_oracle.h: OracleEnv.set_gravity): `gravity`, which acts in the physics, and `gravity_vec`,
which the env layer projects into the body frame and observes. A set whose env layer sees the gravity there is (`observed`) sets both to
g; one that keeps upstream's constant sets only the first. Nothing but the .npz is written into the tree.

    python tests/golden/make_gravity_goldens.py            (CPU only, a few seconds)

Populations and keys are those of env_params.npz (make_envparam_goldens.record): drop, stand, belly; 8 envs x T steps each, per set, free-running.
Besides the trajectories the file holds `sets` [4,6] (offset x y z, tilt theta, azimuth phi, observed) and `rows` [4,8] (g[3], pad,
gravity_vec[3], pad: what nm_set_gravity takes).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gravity.npz")
sys.path.insert(0, HERE)
import make_envparam_goldens as me      # noqa: E402  (the populations, keys and recorder are its record(): one definition)

# (offset x, y, z m/s^2, tilt rad, azimuth rad, observed): nominal; a slope along +x; an offset alone; a steeper slope across both axes whose
# env layer keeps upstream's constant. (Set 3 was first tried at 0.35 and 0.3 rad: there the folded robot of `belly` slides off its legs and
# only 2 env-steps stay above 16 contacts, below the 4 asserted in main(); 0.25 rad is the steepest of the tilts tried that keeps 4.)
SETS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.2, 0.0, 1.0], [0.6, -0.8, 1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.25, 2.2, 0.0]])
G0 = 9.81


def g_of(s):
    """Stated here on its own (the env's derivation is nightmare_v3_env.gravity_from_draw): the nominal vector rotated by theta about the
    horizontal axis at azimuth phi + 90 degrees, plus the offset."""
    off, th, ph = s[0:3], s[3], s[4]
    return np.array([G0 * np.sin(th) * np.cos(ph), G0 * np.sin(th) * np.sin(ph), -G0 * np.cos(th)]) + off


def row_of(s):
    g = g_of(s)
    vec = g if s[5] else np.array([0.0, 0.0, -G0])
    return np.concatenate([g, [0.0], vec, [0.0]])


def rotated(q, v):
    """v rotated by the conjugate of the quaternions q [..., 4] (w x y z): the world vector v in the body frame."""
    w, u = q[..., 0:1], -q[..., 1:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def main():
    rows = np.stack([row_of(s) for s in SETS])
    g = {"sets": SETS, "rows": rows, **me.stacked([me.record(lambda o, r=r: o.set_gravity(r[0:3], r[4:7])) for r in rows])}
    for pop in me.POPS:
        big = (g[f"{pop}_ncon"] > 16).sum(axis=(1, 2))
        con = (g[f"{pop}_ncon"] > 0).sum(axis=(1, 2))
        print(f"{pop}: env-steps with contacts per set {con.tolist()}, with more than 16 contacts {big.tolist()}, resets {g[f'{pop}_done'].sum(axis=(1, 2)).tolist()}")
    # conditions on the reference alone
    assert ((g["belly_ncon"] > 16).sum(axis=(1, 2)) >= 4).all(), "every set must exercise the matrix-free layout on several env-steps"
    assert g["stand_done"].sum() == 0, "no standing env of any set may reset in its recorded steps (tan 0.25 = 0.26 is far below mu = 1)"
    drift = np.abs(g["stand_qpos"][:, -1, :, 0:2] - g["stand_qpos"][:, 0, :, 0:2]).max(axis=(1, 2))
    print("standing robots' largest horizontal drift over the recorded steps per set (m):", drift.tolist())
    # the final standing observation: slots 6..8 are gravity_vec in the body frame - g for the observed sets, upstream's constant for set 3
    for k in range(len(SETS)):
        q = g["stand_qpos"][k, -1][:, 3:7]
        pg = g["stand_obs"][k, -1][:, 6:9]
        own = np.abs(pg - rotated(q, g["rows"][k, 0:3])).max()
        const = np.abs(pg - rotated(q, np.array([0.0, 0.0, -G0]))).max()
        print(f"set {k}: final standing obs[6:9] against g in the body frame {own:.2e}, against the constant {const:.2e}")
        if SETS[k, 5]:
            assert own < 1e-6
        else:
            assert const < 1e-6 and own > 1.0, "the constant-vector variant must really be exercised"
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
