"""StateLog, the host side of cfg.viewer.record_states (reference envs/nightmare_v3_env.py:261-272; reader open_custom_play.py:50-66), and
the C-ABI symbols of the one-launch play path. No GPU needed: nothing here launches a kernel."""
import ctypes
import glob
import os
import pickle

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.016


def _sequence(K=37, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(K, 50))
    rows[:, 49] = 0
    dones = np.zeros(K, np.uint8)
    if K == 37:
        rows[[9, 22], 49] = [1, 3]                   # bad-state resets inside steps 9 and 22: data.time restarts there
        dones[[5, 6, 20, 36]] = 1                    # two dumps back to back, one at the very last step
    return rows, dones


def _read(paths):
    out = []
    for p in paths:
        with open(p, "rb") as f:
            out.append(pickle.load(f))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0]
        np.testing.assert_array_equal(x[1], y[1])
        np.testing.assert_array_equal(x[2], y[2])
        assert np.asarray(x[3]).shape == np.asarray(y[3]).shape == (0,)


def _expected(rows, dones):
    """What _record_state did step by step before the class existed, written out independently: (files, pending)."""
    files, cur, t = [], [], 0.0
    for r, d in zip(rows, dones):
        if d:
            files.append(cur)
            cur = []
        t = DT if r[49] else t + DT
        cur.append((t, r[:25].copy(), r[25:49].copy(), np.zeros(0)))
    return files, cur


@pytest.mark.parametrize("split", [None, [37], [1, 36], [5, 1, 1, 13, 17], [6, 31], [20, 16, 1]])
def test_rows_one_at_a_time_and_in_batches_give_the_same_files(tmp_path, split):
    from nightmare_rl_amd.envs.state_log import StateLog
    rows, dones = _sequence()
    log = StateLog(str(tmp_path / "log"), DT)
    if split is None:
        for r, d in zip(rows, dones):
            log.add(r[:25], r[25:49], int(r[49]), bool(d))
    else:
        assert sum(split) == len(rows)
        i = 0
        for n in split:
            log.add_rows(rows[i:i + n], dones[i:i + n])
            i += n
    files, pending = _expected(rows, dones)
    assert len(log.files) == len(files) == 4
    assert sorted(glob.glob(str(tmp_path / "log" / "*.pkl"))) == log.files          # sorted order = write order
    for got, want in zip(_read(log.files), files):
        _same(got, want)
    _same(log.records, pending)
    # a flagged step's record is the FIRST entry of the next file (upstream dumps, then appends)
    second = _read(log.files)[1]
    np.testing.assert_array_equal(second[0][1], rows[5, :25])
    assert len(second) == 1                                                          # step 6 is flagged too
    np.testing.assert_array_equal(log.records[0][1], rows[36, :25])
    assert len(_read(log.files)[0]) == 5
    # data.time: + dt per step, restarted by a step with a bad-state reset (mj_resetData), not by the env's reset
    times = [r[0] for f in _read(log.files) for r in f] + [r[0] for r in log.records]
    want, t = [], 0.0
    for k in range(len(rows)):
        t = DT if rows[k, 49] else t + DT
        want.append(t)
    assert times == want and times[9] == DT and times[22] == DT and abs(times[8] - 9 * DT) < 1e-15 and abs(times[10] - 2 * DT) < 1e-15
    r0 = log.records[0]
    assert isinstance(r0, tuple) and isinstance(r0[0], float) and r0[1].dtype == np.float64 and r0[1].shape == (25,) and r0[2].shape == (24,)


def test_three_dumps_in_the_same_second_sort_in_write_order(tmp_path):
    from nightmare_rl_amd.envs.state_log import StateLog
    d = tmp_path / "log"
    log = StateLog(str(d), DT, clock=lambda: 1700000000.7)
    rows, _ = _sequence(K=6)
    log.add_rows(rows, [0, 1, 0, 1, 0, 1])
    assert len(log.files) == 3 and len(set(log.files)) == 3
    names = [os.path.basename(p) for p in log.files]
    assert names[0] == "1700000000.pkl" and sorted(names) == names and all(n.startswith("1700000000") and n.endswith(".pkl") for n in names)
    assert sorted(os.listdir(d)) == names
    got = _read(sorted(glob.glob(str(d / "*.pkl"))))
    assert [len(g) for g in got] == [1, 2, 2]
    np.testing.assert_array_equal(got[1][0][1], rows[1, :25])
    np.testing.assert_array_equal(got[2][1][1], rows[4, :25])
    # a second log into the same directory within the same second does not overwrite either
    log2 = StateLog(str(d), DT, clock=lambda: 1700000000.2)
    log2.add_rows(rows[:2], [0, 1])
    assert len(os.listdir(d)) == 4 and sorted(os.listdir(d))[-1] == os.path.basename(log2.files[0])
    # ... and a later second sorts after all of them
    log3 = StateLog(str(d), DT, clock=lambda: 1700000001.0)
    log3.add_rows(rows[:2], [0, 1])
    assert sorted(os.listdir(d))[-1] == "1700000001.pkl"


def test_replaying_the_reference_class_fixture_reproduces_its_files_and_times(tmp_path):
    """tests/golden/env_statelog.npz = what the REFERENCE class pickled when its env 0 timed out (log_*) and what it had logged since
    (pending_*). Its records as the per-step rows, column 0 of its `done` array as the flags: same split, same times (atol 1e-12, the
    bound of test_state_log_pickle_equals_the_reference_class_fixture), arrays unchanged. (The fixture keeps no velocities for the
    pending records: the env's post-step qvel column stands in for them - the class must pass whatever it is given.)"""
    from nightmare_rl_amd.envs.state_log import StateLog
    g = load_golden("env_statelog.npz")
    nlog, npend = len(g["log_time"]), len(g["pending_time"])
    K = g["done"].shape[0]
    assert nlog + npend == K
    qpos = np.concatenate([g["log_qpos"], g["pending_qpos"]])
    qvel = np.concatenate([g["log_qvel"], g["qvel"][nlog:, 0]])
    rows = np.concatenate([qpos, qvel, np.zeros((K, 1))], axis=1)
    dones = g["done"][:, 0]
    assert dones.sum() == 1 and dones[nlog] == 1
    for split in ([1] * K, [K], [7, 13]):
        d = tmp_path / f"log{len(split)}"
        log = StateLog(str(d), float(g["dt"]))
        i = 0
        for n in split:
            log.add_rows(rows[i:i + n], dones[i:i + n])
            i += n
        assert len(log.files) == 1
        rec = _read(log.files)[0]
        r0 = rec[0]
        assert [type(rec).__name__, type(r0).__name__, type(r0[0]).__name__, type(r0[1]).__name__, str(r0[1].dtype), str(r0[1].shape),
                str(r0[2].shape), str(np.asarray(r0[3]).shape)] == [str(x) for x in g["log_types"]]
        assert len(rec) == nlog and len(log.records) == npend
        np.testing.assert_allclose([r[0] for r in rec], g["log_time"], atol=1e-12)
        np.testing.assert_allclose([r[0] for r in log.records], g["pending_time"], atol=1e-12)
        np.testing.assert_array_equal(np.stack([r[1] for r in rec]), g["log_qpos"])
        np.testing.assert_array_equal(np.stack([r[2] for r in rec]), g["log_qvel"])
        np.testing.assert_array_equal(np.stack([r[1] for r in log.records]), g["pending_qpos"])
        np.testing.assert_array_equal(np.stack([r[2] for r in log.records]), qvel[nlog:])
        assert [np.asarray(r[3]).size for r in rec] == g["log_act_size"].tolist()


def test_library_exports_the_play_and_state_log_symbols():
    """Same method as test_abi_and_host.py::test_library_exports_every_declared_symbol, for the entry points of this feature."""
    import re
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    declared = set(re.findall(r"\b(nm_[a-z_0-9]+)\s*\(", hdr))
    new = ["nm_get_state_log", "nm_get_state_log_dones", "nm_play", "nm_play_supported"]
    assert set(new) <= declared and set(new) <= set(_lib.EXPORTS)
    assert "nm_play_args" in hdr and "play.py:118-132" in hdr
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in new if not hasattr(L, s)]
    # host-only entry point: the reference's actor (envs/nightmare_v3_config.py:107) with every activation; nothing else
    L.nm_play_supported.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    dims = (ctypes.c_int32 * 5)(66, 54, 42, 30, 18)
    wide = (ctypes.c_int32 * 5)(66, 256, 42, 30, 18)
    for code in sorted(set(_lib.ACTIVATIONS.values())):
        assert L.nm_play_supported(dims, 4, code) == 1
    assert L.nm_play_supported(wide, 4, 0) == 0 and L.nm_play_supported(dims, 3, 0) == 0 and L.nm_play_supported(dims, 4, 99) == 0
    assert ctypes.sizeof(_lib.NmPlayArgs) == 21 * 8      # 22 fields: steps and deterministic share an 8-byte slot, every other field has its own
