"""Generator of tests/golden/payload.npz: fp64 reference trajectories for per-env base payloads (a point mass dm at r on the base body).

An env with payload (dm, r) behaves as if mjmodel.xml had been recompiled with that mass added to base_link. The oracle takes its model
from nightmare_rl_amd/model/nm_model_data.h at compile time, and a payload changes the base body's mass, COM and inertia, every colliding
body's invweight0 and meaninertia: it is deliberately NOT one of the oracle's per-env rows. A UNIFORM variant of the oracle is the
unchanged oracle source compiled against the header that compile_model.emit_header writes for the modified tables T'
(nightmare_rl_amd/model/payload.py modified_tables: body_mass / body_ipos / body_iquat / body_inertia of body 1 from eigh of I' with a
right-handed axis set, body_invweight0 and meaninertia recomputed at qpos0 through compile_model's own functions) - the independent
path that payload.payload_rows is tested against. For each payload set this script writes that header into a temporary directory,
has oracle.build(header=..., out=...) compile a library against it (the recipe and flags of oracle/Makefile) and binds it with
OracleEnv(lib_path=...). Nothing but the .npz is written into the tree.

    python tests/golden/make_payload_goldens.py            (CPU only, a few seconds; four library builds)

Populations (8 envs x T steps each, per set, free-running; every step's start state is the previous step's end state):
    drop   random actions while the robot falls from the initial pose and lands
    stand  zero actions after the robot has settled on its feet
    belly  the robot lying on folded legs while its servos hold the pose (the initial states of env_manycontacts.npz): of 80 steps the T
           consecutive ones with the most env-steps above 16 contacts (the matrix-free constraint layout)
Besides the trajectories the file holds `sets` [4,4] (dm, rx, ry, rz), `rows` [4,20] (the body rows of the four sets, by the per-env path)
and `stand_height` [4]: the mean base-body COM height of the standing population at the start of its recorded steps.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "payload.npz")
# (dm kg, r m): none, a battery forward and above, a lighter base plate, a camera mast aft - all admissible, all with distinct constants
SETS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])
sys.path.insert(0, HERE)
import make_envparam_goldens as me      # noqa: E402  (the populations, keys and recorder are its record(): one definition)

POPS, N, T, SEED = me.POPS, me.N, me.T, me.SEED


def payload_lib(tmp, dm, r):
    """The one place a library is built: the oracle against the header of the model recompiled with (dm, r) on the base. Returns the
    library and the body row of those tables."""
    sys.path.insert(0, ROOT)
    from nightmare_rl_amd.model import compile_model as cm, payload as pl
    from oracle import oracle as orc
    d = tempfile.mkdtemp(dir=tmp)
    Tv = pl.modified_tables(float(dm), np.asarray(r, np.float64))
    cm.emit_header(Tv, os.path.join(d, "nm_model_data.h"))
    return orc.build(header=os.path.join(d, "nm_model_data.h"), out=os.path.join(d, "libnm_oracle.so")), pl.row_of_tables(Tv)


def main():
    tmp = tempfile.mkdtemp(prefix="nm_payload_")
    try:
        parts = []
        rows = []
        for k, pay in enumerate(SETS):
            lib, row = payload_lib(tmp, pay[0], pay[1:])
            rows.append(row)
            parts.append(me.record(lib_path=lib))
        g = {"sets": SETS, "rows": np.stack(rows), **me.stacked(parts)}
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
    main()
