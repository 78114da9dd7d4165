"""What the torque-limit tests share (test infrastructure): the mixed batch of tests/golden/torque.npz - env e takes set e % 5, so the two
envs of a wave always differ - and the numpy restatement of the clamp and the mask."""
import numpy as np

POPS = ("drop", "stand")
NSET = 5


def set_of(n):
    return np.arange(n) % NSET


def mixed(g, key, t, n=8):
    """[n, ...]: row e of step t from the recording of set e % 5."""
    e = np.arange(n)
    return g[key][set_of(n), t, e % 8]


def mixed_rows(g, n=8):
    """([n,3] limits, [n] kv) of the mixed batch."""
    return g["sets"][set_of(n)], g["kv"][set_of(n)]


def clamp_and_mask(f, fmax):
    """The semantics in numpy, compares and selects: (f', d) for forces [..., 18] and limits [..., 3] (word k limits joint 3 leg + k)."""
    lim = np.tile(np.asarray(fmax, np.float64), 6) if np.ndim(fmax) == 1 else np.tile(np.asarray(fmax, np.float64), (1, 6))
    fc = np.where(f > lim, lim, np.where(f < -lim, -lim, f))
    return fc, (np.abs(f) < lim).astype(np.float64)
