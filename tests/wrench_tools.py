"""What the wrench tests share (test infrastructure): the mixed batch of tests/golden/wrench.npz - env e takes set e % 5, so the two envs
of a wave always differ - and the numpy restatements of the schedule and of the draw over oracle.rand_u24."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POPS = ("drop", "stand")
NSET = 5
MASK = 2 ** 64 - 1


def set_of(n):
    return np.arange(n) % NSET


def mixed(g, key, t, n=8):
    """[n, ...]: row e of step t from the recording of set e % 5."""
    e = np.arange(n)
    return g[key][set_of(n), t, e % 8]


def mixed_wrench(g, n=8):
    """[n,6] (F, tau) of the mixed batch."""
    return g["sets"][set_of(n)]


def mixed_payload(g, n=8):
    """(dm [n], r [n,3]) of the mixed batch: set 3 carries the payload."""
    p = g["payload"][set_of(n)]
    return p[:, 0].copy(), p[:, 1:].copy()


def wrench_key():
    """nm::kWrenchKey as nm_core.h states it."""
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_core.h")).read()
    return int(re.search(r"kWrenchKey = (0x[0-9A-Fa-f]+)ull", src).group(1), 16)


def draw_restated(seed, env_ids, q, maxima, npdt):
    """[n,6] (F, tau) of window q: v = (2u - 1) max[axis] in the env's precision, u = rand_u24(seed + kWrenchKey, global env id,
    6 q + axis) 2^-24 (24 bits: 2u - 1 is exact in either precision, so v is rounded once)."""
    from oracle import oracle as orc
    mx = np.asarray(maxima, np.float64).astype(npdt)
    out = np.empty((len(env_ids), 6), npdt)
    for axis in range(6):
        u = np.array([orc.rand_u24((seed + wrench_key()) & MASK, int(e), (6 * q + axis) & 0xFFFFFFFF) for e in env_ids]).astype(npdt)
        out[:, axis] = (npdt(2) * u - npdt(1)) * mx[axis]
    assert out.dtype == npdt
    return out


def schedule_restated(seed, env_ids, interval, duration, maxima, npdt, first, last, rows0=None):
    """The rows ([n,6]) the physics of steps first..last-1 reads, as a list: at the start of step s a fresh draw if s >= interval and
    s % interval == 0, zero if s >= interval and s % interval == duration (duration < interval), unchanged otherwise. rows0: what holds
    before step `first` (None: what nm_set_wrench_schedule installs at start_step = first)."""
    n = len(env_ids)
    if rows0 is None:
        inside = first >= interval and first % interval < duration
        rows0 = draw_restated(seed, env_ids, first // interval, maxima, npdt) if inside else np.zeros((n, 6), npdt)
    rows, out = np.asarray(rows0, npdt), []
    for s in range(first, last):
        if s >= interval and s % interval == 0:
            rows = draw_restated(seed, env_ids, s // interval, maxima, npdt)
        elif s >= interval and duration < interval and s % interval == duration:
            rows = np.zeros((n, 6), npdt)
        out.append(rows)
    return out
