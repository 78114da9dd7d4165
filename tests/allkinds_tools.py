"""What tests/test_allkinds_emulated.py (CPU, the emulation shim) and tests/test_gpu_allkinds.py (the library) share about the combined
fixture tests/golden/allkinds.npz (make_allkinds_goldens.py): all seven kinds of per-env rows on at once. Test infrastructure, like
allrand_tools.py: the loader, which env of a batch takes which combined set, the rows of every kind for such a batch, and where the
reference itself says a kind matters."""
import numpy as np

from conftest import load_golden

POPS = ("drop", "stand", "belly")
ABLATIONS = ("gravity", "friction", "payload", "latency", "rate", "d_gain", "torque", "wrench")      # the servo row split in two
DEFAULT = dict(gravity=np.array([0.0, 0.0, -9.81, 0.0, 0.0, 0.0, -9.81, 0.0]), friction=np.array([1.0, 20.0, 0.8]), payload=np.zeros(4),
               torque=np.full(3, np.inf), wrench=np.zeros(6))
REGIONS = ("gravity", "friction", "body", "latency", "servo", "torque", "wrench")      # one per region of the row block


def load():
    """The fixture as a dict, with the three keys its generator leaves out (it asserts the equalities) derived again."""
    g = dict(load_golden("allkinds.npz"))
    for pop in POPS:
        g[f"{pop}_dof_pos"], g[f"{pop}_dof_vel"] = g[f"{pop}_qpos"][..., 7:], g[f"{pop}_qvel"][..., 6:]
        g[f"{pop}_act"] = g[f"{pop}_hist"][:, :, :, 0].astype(np.float64)
    return g


def set_of(n):
    """Combined set of env e: neighbours in a wave (2w, 2w + 1) always hold different sets, and every set meets every slot."""
    e = np.arange(n)
    return (e + e // 4) % 4


def rows_of(g, sets, without=None):
    """Per env of a batch whose env e takes env e % 8 of combined set sets[e]: gravity [n,8], friction [n,3], payload [n,4] (dm, r),
    body [n,20] (the host's batched derivation from the payloads), latency [n], servo [n,2] (rate, d_gain), torque [n,3] and
    wrench [n,6] (F, tau) - with the ablation `without` (one of ABLATIONS) at its default VALUES."""
    from nightmare_rl_amd.model import payload
    n = len(sets)
    ev = np.arange(n) % 8
    r = dict(gravity=g["grav_rows"][sets], friction=g["envp_rows"][sets], payload=g["payloads"][sets], latency=g["delays"][ev].astype(np.int32),
             servo=g["servo_rows"][ev].copy(), torque=g["torque_rows"][sets], wrench=g["wrench_rows"][sets])
    if without == "latency":
        r["latency"] = np.zeros(n, np.int32)
    elif without == "rate":
        r["servo"][:, 0] = np.inf
    elif without == "d_gain":
        r["servo"][:, 1] = 0.0
    elif without is not None:
        r[without] = np.tile(DEFAULT[without], (n, 1))
    r["body"] = payload.payload_rows(r["payload"][:, 0], r["payload"][:, 1:])
    return r


def nondefault(g, sets, kind):
    """[n] bool: env e carries a non-default value of that kind (one of ABLATIONS)."""
    ev = np.arange(len(sets)) % 8
    if kind == "latency":
        return g["delays"][ev] > 0
    if kind == "rate":
        return np.isfinite(g["servo_rows"][ev, 0])
    if kind == "d_gain":
        return g["servo_rows"][ev, 1] != 0
    if kind == "torque":
        return np.isfinite(g["torque_rows"][sets]).any(axis=1)
    if kind == "wrench":
        return (g["wrench_rows"][sets] != 0).any(axis=1)
    return g["sets"][sets, ABLATIONS.index(kind)] != 0


def sensitive(g, sets, kind, pop):
    """[n] bool: the REFERENCE with that one kind at its default leaves env e's recorded trajectory (by more than 1e-5 in qpos; every other
    env by nothing, which the generator asserts). Recorded for `drop` and `stand`."""
    return g["sensitive"][ABLATIONS.index(kind), sets, ("drop", "stand").index(pop), np.arange(len(sets)) % 8].astype(bool)
