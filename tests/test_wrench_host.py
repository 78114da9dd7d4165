"""The external wrench on the base (nm_set_base_wrench / nm_get_base_wrench / nm_set_wrench_schedule / nm_get_wrench_schedule, the optional
cfg.domain_rand.external_wrench): what needs no device - the exports with their ctypes binding and header text, every refusal that comes
before the handle is looked at, the config parsing with every ValueError, that the shipped config tree is unchanged, and the numpy
restatements of the schedule and of the draw over oracle.rand_u24 that tests/test_gpu_wrench.py holds the device against. (The admission
of rows is the host's nmrows::wrench_rows_fault: tests/test_wrench_emulated.py drives it through the emulation shim.)"""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

from wrench_tools import draw_restated, schedule_restated, wrench_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def test_library_exports_the_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_set_base_wrench", "nm_get_base_wrench", "nm_set_wrench_schedule", "nm_get_wrench_schedule"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d3, i64 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 3), ctypes.c_int64
    assert L.nm_set_base_wrench.argtypes == [vp] * 3
    assert L.nm_get_base_wrench.argtypes == [vp] * 3
    assert L.nm_set_wrench_schedule.argtypes == [vp, i64, i64, d3, d3, ctypes.c_uint64]
    assert L.nm_get_wrench_schedule.argtypes == [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), d3, d3, ctypes.POINTER(ctypes.c_uint64)]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_base_wrench\(nm_env\* env, const void\* rows_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_base_wrench\(nm_env\* env, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_set_wrench_schedule\(nm_env\* env, int64_t interval_steps, int64_t duration_steps, const double max_force\[3\], "
                     r"const double max_torque\[3\],\s+uint64_t start_step\);", hdr)
    assert re.search(r"int nm_get_wrench_schedule\(nm_env\* env, int64_t\* interval_steps, int64_t\* duration_steps, double max_force\[3\], "
                     r"double max_torque\[3\], uint64_t\* step\);", hdr)
    # the header names what the entry points stand for and states the closed form and the schedule
    for words in ("xfrc_applied", "qfrc_smooth[0:3] += F", "Rb' tau + ipos x (Rb' F)", "M + h kv D does not change", "s % interval_steps == duration_steps",
                  '"WRENCH"', "6 q + axis", "nm_step_physics"):
        assert words in hdr, words


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_base_wrench", "nm_get_base_wrench"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    f, t = (ctypes.c_double * 3)(1.0, 1.0, 1.0), (ctypes.c_double * 3)(0.1, 0.1, 0.1)
    assert L.nm_set_wrench_schedule(None, 3, 2, ctypes.byref(f), ctypes.byref(t), 0) != 0
    assert b"nm_set_wrench_schedule" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert L.nm_set_wrench_schedule(None, 0, 0, None, None, 0) != 0 and b"env is NULL" in L.nm_last_error()      # off needs no maxima, but a handle
    iv, du, st = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_uint64(7)
    assert L.nm_get_wrench_schedule(None, ctypes.byref(iv), ctypes.byref(du), None, None, ctypes.byref(st)) != 0
    assert b"nm_get_wrench_schedule" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert (iv.value, du.value, st.value) == (7, 7, 7)


@pytest.mark.parametrize("iv,du,force,torque,word", [
    (3, 2, (NAN, 1, 1), (0, 0, 0), b"max_force must be finite and >= 0"),
    (3, 2, (1, INF, 1), (0, 0, 0), b"max_force must be finite and >= 0"),
    (3, 2, (1, 1, -0.5), (0, 0, 0), b"max_force must be finite and >= 0"),
    (3, 2, (1, 1, 1), (0, NAN, 0), b"max_torque must be finite and >= 0"),
    (3, 2, (1, 1, 1), (-1, 0, 0), b"max_torque must be finite and >= 0"),
    (3, 2, (1, 1, 1), (0, 0, -INF), b"max_torque must be finite and >= 0"),
    (3, 0, (1, 1, 1), (0, 0, 0), b"duration_steps must lie in [1, interval_steps]"),
    (3, -1, (1, 1, 1), (0, 0, 0), b"duration_steps must lie in [1, interval_steps]"),
    (3, 4, (1, 1, 1), (0, 0, 0), b"duration_steps must lie in [1, interval_steps]"),
    (2 ** 31, 1, (1, 1, 1), (0, 0, 0), b"2^31 steps or more"),
    (2 ** 40, 1, (1, 1, 1), (0, 0, 0), b"2^31 steps or more"),
    (-1, 1, (1, 1, 1), (0, 0, 0), b"interval_steps must be >= 0"),
])
def test_bad_schedules_are_refused_before_the_handle_is_looked_at(L, iv, du, force, torque, word):
    f, t = (ctypes.c_double * 3)(*force), (ctypes.c_double * 3)(*torque)
    assert L.nm_set_wrench_schedule(None, iv, du, ctypes.byref(f), ctypes.byref(t), 0) != 0
    assert word in L.nm_last_error() and b"env is NULL" not in L.nm_last_error(), L.nm_last_error()


def test_missing_maxima_are_refused_before_the_handle(L):
    t = (ctypes.c_double * 3)(0.1, 0.1, 0.1)
    assert L.nm_set_wrench_schedule(None, 3, 2, None, ctypes.byref(t), 0) != 0 and b"max_force / max_torque is NULL" in L.nm_last_error()
    assert L.nm_set_wrench_schedule(None, 2 ** 31 - 1, 2 ** 31 - 1, ctypes.byref(t), ctypes.byref(t), 0) != 0      # the largest interval passes the checks
    assert b"env is NULL" in L.nm_last_error()


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(**kw):
    return types.SimpleNamespace(domain_rand=types.SimpleNamespace(**kw))


def test_the_config_names_are_parsed():
    from nightmare_rl_amd.envs.nightmare_v3_env import wrench_config as f
    dt = 0.008 * 2
    assert f(types.SimpleNamespace(), dt) is None
    assert f(_cfg(), dt) is None
    assert f(_cfg(external_wrench=False, wrench_interval_s=1.0, wrench_duration_s=0.5, max_wrench_force=3.0), dt) is None
    assert f(_cfg(external_wrench=True, wrench_interval_s=8.0, wrench_duration_s=0.5, max_wrench_force=3.0), dt) == (500, 31, [3.0] * 3, [0.0] * 3)      # 0.5 / 0.016 = 31.25
    assert f(_cfg(external_wrench=True, wrench_interval_s=0.048, wrench_duration_s=0.032, max_wrench_torque=[0.1, 0.2, 0.3]), dt) == (3, 2, [0.0] * 3, [0.1, 0.2, 0.3])      # push_config's rounding: 0.048 / 0.016 = 2.9999999999999996
    assert f(_cfg(external_wrench=True, wrench_interval_s=0.016, wrench_duration_s=0.016, max_wrench_force=(1, 2, 3), max_wrench_torque=0.0), dt) == (1, 1, [1.0, 2.0, 3.0], [0.0] * 3)
    assert f(_cfg(external_wrench=True, wrench_interval_s=0.064, wrench_duration_s=0.064, max_wrench_force=0, max_wrench_torque=0.5), 0.032) == (2, 2, [0.0] * 3, [0.5] * 3)


def test_every_value_error_of_the_config():
    from nightmare_rl_amd.envs.nightmare_v3_env import wrench_config as f
    dt = 0.016
    ok = dict(external_wrench=True, wrench_interval_s=1.0, wrench_duration_s=0.5, max_wrench_force=3.0)
    for name in ("wrench_interval_s", "wrench_duration_s"):
        for bad in (0.015, 0.0, -1.0, NAN, 2.0 ** 31):      # below one step ... more than 2^31 steps
            with pytest.raises(ValueError, match=name):
                f(_cfg(**dict(ok, **{name: bad})), dt)
        with pytest.raises(ValueError, match=name):
            f(_cfg(**{k: v for k, v in ok.items() if k != name}), dt)
    with pytest.raises(ValueError, match="wrench_interval_s"):
        f(_cfg(**dict(ok, wrench_interval_s=0.016)), 0.032)      # one step of another decimation
    with pytest.raises(ValueError, match="wrench_duration_s must not exceed"):
        f(_cfg(**dict(ok, wrench_duration_s=1.5)), dt)
    for name in ("max_wrench_force", "max_wrench_torque"):
        for bad in (-1.0, NAN, INF, "strong", [1.0, 2.0], [1.0, 2.0, -3.0], [1.0, 2.0, 3.0, 4.0]):
            with pytest.raises(ValueError, match=name):
                f(_cfg(**dict(ok, **{name: bad})), dt)
    with pytest.raises(ValueError, match="max_wrench_force or max_wrench_torque"):
        f(_cfg(external_wrench=True, wrench_interval_s=1.0, wrench_duration_s=0.5), dt)


def test_the_shipped_config_tree_is_unchanged():
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    from nightmare_rl_amd.envs.nightmare_v3_env import wrench_config
    cfg = NightmareV3Config()
    assert not hasattr(cfg, "domain_rand") and wrench_config(cfg, 0.016) is None
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    assert "wrench" not in json.dumps(golden)
    ours = {"NightmareV3Config": class_to_dict(cfg), "NightmareV3ConfigPPO": class_to_dict(NightmareV3ConfigPPO())}
    assert "wrench" not in json.dumps(ours)
    assert list(ours["NightmareV3Config"]) == list(golden["NightmareV3Config"]) and ours["NightmareV3ConfigPPO"] == golden["NightmareV3ConfigPPO"]

    class Tethered(NightmareV3Config):
        class domain_rand:
            external_wrench, wrench_interval_s, wrench_duration_s, max_wrench_force = True, 8.0, 0.5, [5.0, 5.0, 2.0]

    assert wrench_config(Tethered(), 0.016) == (500, 31, [5.0, 5.0, 2.0], [0.0] * 3)


def test_the_command_line_flags_exist():
    src = open(os.path.join(ROOT, "train.py")).read()
    for flag in ("--wrench-interval-s", "--wrench-duration-s", "--wrench-force", "--wrench-torque"):
        assert f'"{flag}"' in src, flag
    assert "external_wrench, wrench_interval_s = " in src


def test_the_pooled_kinds_stay_six():
    """Re-draws at reset do not know the wrench: nmrows::kKinds, the 41 words and RESET_POOL_KINDS keep their values."""
    rows = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_env_rows.h")).read()
    assert "constexpr int kKinds = 6;" in rows and "kWrench = 6" in rows and "bool on[7]" in rows
    rr = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_reset_rows.h")).read()
    assert "kResetRowKinds = 6" in rr and "kResetRowWords == 41" in rr
    from nightmare_rl_amd.envs import nightmare_v3_env as ev
    assert len(ev.RESET_POOL_KINDS) == 6 and not any("wrench" in k for k in ev.RESET_POOL_KINDS)


# ---------------------------------------------------------------------------------------------------------------- the restatements
def test_the_restated_draw_is_keyed_by_the_global_env_id_and_the_window():
    """What the device is held against (tests/test_gpu_wrench.py): in range, six independent axes, another draw per window, and a shard
    with env_offset = 8 draws the slice [8:16] of a 16-env draw."""
    assert wrench_key() == int.from_bytes(b"WRENCH", "big")
    mx = [4.0, 4.0, 2.0, 0.3, 0.0, 0.5]
    for npdt in (np.float32, np.float64):
        w = draw_restated(5, np.arange(100, 164), 1, mx, npdt)
        for a in (0, 1, 2, 3, 5):
            assert w[:, a].min() >= -npdt(mx[a]) and w[:, a].max() < npdt(mx[a]) and np.unique(w[:, a]).size > 50
            assert w[:, a].min() < 0 < w[:, a].max()
        assert (w[:, 4] == 0).all()      # a zero maximum pins an axis
        assert np.abs(w[:, 0] - w[:, 1]).max() > 1.0      # independent draws, not one draw scaled
        assert np.abs(w - draw_restated(5, np.arange(100, 164), 2, mx, npdt)).max() > 1.0
        np.testing.assert_array_equal(draw_restated(5, np.arange(8, 16), 3, mx, npdt), draw_restated(5, np.arange(16), 3, mx, npdt)[8:])
    # (2u - 1) max is rounded once: the float32 draw is the rounded float64 draw wherever max is a float32 number
    np.testing.assert_array_equal(draw_restated(5, np.arange(16), 1, [4.0, 4.0, 2.0, 0.25, 0.0, 0.5], np.float32),
                                  draw_restated(5, np.arange(16), 1, [4.0, 4.0, 2.0, 0.25, 0.0, 0.5], np.float64).astype(np.float32))


def test_the_restated_schedule_opens_and_closes_windows():
    """interval 3, duration 2: nothing before step 3; windows open at steps 3 and 6 (draws of windows 1 and 2) and close at steps 5 and 8;
    duration = interval never zeroes; a schedule picked up at start_step continues the one that ran from 0."""
    mx, ids = [4.0, 3.0, 2.0, 0.3, 0.2, 0.1], np.arange(8)
    rows = schedule_restated(5, ids, 3, 2, mx, np.float32, 0, 10)
    zero, w1, w2, w3 = np.zeros((8, 6), np.float32), *(draw_restated(5, ids, q, mx, np.float32) for q in (1, 2, 3))
    for s, want in enumerate([zero, zero, zero, w1, w1, zero, w2, w2, zero, w3]):
        np.testing.assert_array_equal(rows[s], want, err_msg=f"step {s}")
    full = schedule_restated(5, ids, 3, 3, mx, np.float32, 0, 10)
    for s, want in enumerate([zero, zero, zero, w1, w1, w1, w2, w2, w2, w3]):
        np.testing.assert_array_equal(full[s], want, err_msg=f"duration = interval, step {s}")
    for start in range(10):
        for got, want in zip(schedule_restated(5, ids, 3, 2, mx, np.float32, start, 10), rows[start:]):
            np.testing.assert_array_equal(got, want, err_msg=f"start_step {start}")
    # rows set by hand before a window stay until the schedule's first event
    mine = np.ones((8, 6), np.float32)
    kept = schedule_restated(5, ids, 3, 2, mx, np.float32, 0, 4, rows0=mine)
    assert all((r == 1).all() for r in kept[:3]) and (kept[3] == w1).all()
