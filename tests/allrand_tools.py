"""What tests/test_allrand_emulated.py (CPU, the emulation shim) and tests/test_gpu_allrand.py (the library) share about the combined
fixture tests/golden/allrand.npz (make_allrand_goldens.py): all four kinds of per-env rows on at once. Test infrastructure, like
rows_walk.py: the loader, which env of a batch takes which combined set, and the rows of every kind for such a batch."""
import numpy as np

from conftest import load_golden

POPS = ("drop", "stand", "belly")
KINDS = ("gravity", "friction", "payload", "latency")
DEFAULT = dict(gravity=np.array([0.0, 0.0, -9.81, 0.0, 0.0, 0.0, -9.81, 0.0]), friction=np.array([1.0, 20.0, 0.8]), payload=np.zeros(4))


def load():
    """The fixture as a dict, with the two keys its generator leaves out (it asserts the equality) derived again."""
    g = dict(load_golden("allrand.npz"))
    for pop in POPS:
        g[f"{pop}_dof_pos"], g[f"{pop}_dof_vel"] = g[f"{pop}_qpos"][..., 7:], g[f"{pop}_qvel"][..., 6:]
    return g


def set_of(n):
    """Combined set of env e: neighbours in a wave (2w, 2w + 1) always hold different sets, and every set meets every slot."""
    e = np.arange(n)
    return (e + e // 4) % 4


def rows_of(g, sets, without=None):
    """Per env of a batch whose env e takes env e % 8 of combined set sets[e]: gravity [n,8], friction [n,3], payload [n,4] (dm, r),
    body [n,20] (the host's batched derivation from the payloads) and latency [n] - with the kind `without` at its default VALUES."""
    from nightmare_rl_amd.model import payload
    n = len(sets)
    r = dict(gravity=g["grav_rows"][sets], friction=g["envp_rows"][sets], payload=g["payloads"][sets], latency=g["delays"][np.arange(n) % 8].astype(np.int32))
    if without == "latency":
        r["latency"] = np.zeros(n, np.int32)
    elif without is not None:
        r[without] = np.tile(DEFAULT[without], (n, 1))
    r["body"] = payload.payload_rows(r["payload"][:, 0], r["payload"][:, 1:])
    return r


def nondefault(g, sets, kind):
    """[n] bool: env e carries a non-default value of that kind."""
    if kind == "latency":
        return g["delays"][np.arange(len(sets)) % 8] > 0
    return g["sets"][sets, KINDS.index(kind)] != 0
