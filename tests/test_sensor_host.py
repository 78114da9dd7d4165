"""The per-env sensor model (nm_set_sensor / nm_get_sensor / nm_draw_sensor / nm_sensor_draw_values / nm_get_sensor_state /
nm_set_sensor_state / nm_get_true_obs, the optional cfg.domain_rand): what needs no device - the exports and their binding, the refusals
that come before any device call, the config parsing, and the draw through the library's host function."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import sensor_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nm_set_sensor", "nm_get_sensor", "nm_draw_sensor", "nm_sensor_draw_values", "nm_get_sensor_state", "nm_set_sensor_state", "nm_get_true_obs")
KINDS = ("lin_vel", "ang_vel", "gravity", "dof_pos", "dof_vel")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def _draw(L, seed, env, lo, hi, bmax):
    d, b = (C.c_int32 * 2)(), (C.c_float * 66)()
    rc = L.nm_sensor_draw_values(seed, env, C.byref((C.c_int32 * 2)(*lo)), C.byref((C.c_int32 * 2)(*hi)), C.byref((C.c_double * 5)(*bmax)), C.byref(d), C.byref(b))
    assert rc == 0, L.nm_last_error()
    return np.array(d[:], np.int32), np.array(b[:], np.float32)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.EXPORTS and re.search(r"int %s\(" % name, hdr), name
    assert re.search(r"int nm_set_sensor\(nm_env\* env, const int32_t\* delays_dev, const float\* bias_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_sensor\(nm_env\* env, const int32_t lo\[2\], const int32_t hi\[2\], const double bias_max\[5\], void\* stream\);", hdr)
    assert "There is no reference line" in hdr and "min(d_g, n - 1)" in hdr and "passed through bit for bit" in hdr
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_sensor.h")).read()
    m = re.search(r"kSensorKey = (0x[0-9A-Fa-f]+)ull", src)
    assert m and int(m.group(1), 16) == sn.SENSOR_KEY and sn.SENSOR_KEY.to_bytes(5, "big") == b"SENSO"
    assert re.search(r"kSensorMaxDelay = 3, kSensorSlots = 4\b", src)


def test_a_null_handle_and_bad_bounds_are_refused_by_name(L):
    for fn in ("nm_set_sensor", "nm_get_sensor_state", "nm_set_sensor_state", "nm_get_true_obs"):
        assert getattr(L, fn)(None, None, None) != 0 if fn != "nm_set_sensor" else L.nm_set_sensor(None, None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    i2, d5 = lambda *v: C.byref((C.c_int32 * 2)(*v)), lambda *v: C.byref((C.c_double * 5)(*v))
    assert L.nm_draw_sensor(None, i2(0, 0), i2(3, 3), d5(0, 0, 0, 0, 0), None) != 0 and b"env is NULL" in L.nm_last_error()
    for lo, hi, mx, word in (((-1, 0), (2, 2), (0,) * 5, b"lo < 0"), ((0, 3), (3, 2), (0,) * 5, b"lo > hi"), ((0, 0), (3, 4), (0,) * 5, b"above 3"),
                             ((0, 0), (1, 1), (0, -0.1, 0, 0, 0), b"ang_vel"), ((0, 0), (1, 1), (0, 0, 0, float("nan"), 0), b"dof_pos"),
                             ((0, 0), (1, 1), (0, 0, 0, 0, float("inf")), b"dof_vel")):
        assert L.nm_draw_sensor(None, i2(*lo), i2(*hi), d5(*mx), None) != 0
        assert word in L.nm_last_error() and b"env is NULL" not in L.nm_last_error(), L.nm_last_error()
        d, b = (C.c_int32 * 2)(), (C.c_float * 66)()
        assert L.nm_sensor_draw_values(1, 0, i2(*lo), i2(*hi), d5(*mx), C.byref(d), C.byref(b)) != 0 and word in L.nm_last_error()


def test_host_draw_stays_in_range_reaches_both_ends_and_is_keyed(L):
    bmax = (0.3, 0.05, 0.02, 0.04, 1.5)
    lo, hi = (0, 1), (3, 2)
    D, B = zip(*[_draw(L, 7, e, lo, hi, bmax) for e in range(4096)])
    D, B = np.stack(D), np.stack(B)
    assert D[:, 0].min() == 0 and D[:, 0].max() == 3 and D[:, 1].min() == 1 and D[:, 1].max() == 2
    assert set(np.unique(D[:, 0])) == {0, 1, 2, 3}
    assert np.array_equal(B[:, sn.PASS], np.zeros((4096, sn.PASS.size), np.float32))       # columns 9..11 and 48..65
    for k, name in enumerate(KINDS):
        cols, m = sn.KIND_COLS[name], np.float32(bmax[k])
        assert (np.abs(B[:, cols]) <= m).all() and np.abs(B[:, cols]).max() > 0.99 * m and B[:, cols].min() < 0 < B[:, cols].max(), name
    # another seed or another env id is another draw; the same key is the same draw
    d0, b0 = _draw(L, 7, 100, lo, hi, bmax)
    assert np.array_equal(b0, B[100]) and np.array_equal(d0, D[100])
    assert not np.array_equal(_draw(L, 8, 100, lo, hi, bmax)[1], b0) and not np.array_equal(_draw(L, 7, 101, lo, hi, bmax)[1], b0)
    assert not np.array_equal(np.stack([_draw(L, 8, e, lo, hi, bmax)[0] for e in range(64)]), D[:64])
    # lo == hi pins the delay; a zero maximum pins the bias to zero
    for v in range(4):
        d, b = _draw(L, 3, 11, (v, v), (v, v), (0, 0, 0, 0, 0))
        assert d.tolist() == [v, v] and not b.any()


def test_host_draw_against_its_restatement(L):
    """bias = (2 u - 1) max in float32, u = 24 bits x 2^-24 from the counter RNG keyed by (seed + "SENSO", global env id, column); the delay
    of group g is lo + floor(u (hi - lo + 1)) with the bits of word 66 + g (tests/test_latency_host.py restates the same rule)."""
    from oracle import oracle as orc
    bmax = (0.3, 0.05, 0.02, 0.04, 1.5)
    for seed, env in ((7, 0), (7, 5000), (2 ** 40 + 3, 12)):
        d, b = _draw(L, seed, env, (0, 1), (3, 3), bmax)
        u = np.array([orc.rand_u24((seed + sn.SENSOR_KEY) & (2 ** 64 - 1), env, w) for w in range(68)], np.float64)
        want = np.zeros(66, np.float32)
        for k, name in enumerate(KINDS):
            cols = sn.KIND_COLS[name]
            want[cols] = (np.float32(2.0) * u[cols].astype(np.float32) - np.float32(1.0)) * np.float32(bmax[k])
        assert np.array_equal(b, want)
        assert d.tolist() == [0 + int(np.floor(u[66] * 4)), 1 + int(np.floor(u[67] * 3))]


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(**kw):
    scales = types.SimpleNamespace(lin_vel=2.0, ang_vel=0.25, dof_pos=1.0, dof_vel=0.05)
    return types.SimpleNamespace(domain_rand=types.SimpleNamespace(**kw), normalization=types.SimpleNamespace(obs_scales=scales))


def test_optional_domain_rand_is_parsed():
    from nightmare_rl_amd.envs.nightmare_v3_env import sensor_config as f
    assert f(types.SimpleNamespace()) == (None, None, None)
    assert f(_cfg(randomize_obs_latency=False, imu_latency_range=[0, 3], randomize_sensor_bias=False, sensor_bias={"lin_vel": 1})) == (None, None, None)
    assert f(_cfg(randomize_obs_latency=True, imu_latency_range=[0, 3])) == ((0, 3), None, None)
    assert f(_cfg(randomize_obs_latency=True, joint_latency_range=(1.0, 2.0), imu_latency_range=[0, 0])) == ((0, 0), (1, 2), None)
    b = f(_cfg(randomize_sensor_bias=True, sensor_bias={"lin_vel": 0.1, "ang_vel": 0.2, "gravity": 0.03, "dof_pos": 0.02, "dof_vel": 2.0}))[2]
    assert b == {"lin_vel": 0.1 * 2.0, "ang_vel": 0.2 * 0.25, "gravity": 0.03, "dof_pos": 0.02, "dof_vel": 2.0 * 0.05}      # x obs_scales; gravity has none

    class bias_class:
        ang_vel, dof_pos = 0.4, 0.0
    assert f(_cfg(randomize_sensor_bias=True, sensor_bias=bias_class))[2] == {"ang_vel": 0.1, "dof_pos": 0.0}
    assert f(_cfg(randomize_sensor_bias=True, sensor_bias=bias_class()))[2] == {"ang_vel": 0.1, "dof_pos": 0.0}


def test_every_refusal_of_the_config():
    from nightmare_rl_amd.envs.nightmare_v3_env import sensor_config as f
    with pytest.raises(ValueError, match="needs imu_latency_range or joint_latency_range"):
        f(_cfg(randomize_obs_latency=True))
    for bad in ([3, 1], [-1, 2], [0.5, 2], [0, float("inf")], [float("nan"), 1], 3, [1, 2, 3]):
        for name in ("imu_latency_range", "joint_latency_range"):
            with pytest.raises(ValueError, match=name):
                f(_cfg(randomize_obs_latency=True, **{name: bad}))
    with pytest.raises(ValueError, match="needs sensor_bias"):
        f(_cfg(randomize_sensor_bias=True))
    with pytest.raises(ValueError, match="at least one"):
        f(_cfg(randomize_sensor_bias=True, sensor_bias={}))
    with pytest.raises(ValueError, match="unknown kinds .*commands"):
        f(_cfg(randomize_sensor_bias=True, sensor_bias={"commands": 0.1}))
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="sensor_bias.dof_vel"):
            f(_cfg(randomize_sensor_bias=True, sensor_bias={"dof_vel": bad}))


def test_a_user_subclass_adds_the_model_and_the_shipped_config_does_not_have_it():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import latency_config, sensor_config

    class SensedConfig(NightmareV3Config):
        class domain_rand:
            randomize_obs_latency, imu_latency_range, joint_latency_range = True, [1, 3], [0, 1]
            randomize_sensor_bias = True

            class sensor_bias:
                ang_vel, dof_pos = 0.2, 0.03

    s = NightmareV3Config.normalization.obs_scales
    assert sensor_config(SensedConfig()) == ((1, 3), (0, 1), {"ang_vel": 0.2 * s.ang_vel, "dof_pos": 0.03 * s.dof_pos})
    assert latency_config(SensedConfig()) is None
    assert not hasattr(NightmareV3Config, "domain_rand") and sensor_config(NightmareV3Config()) == (None, None, None)


def test_command_line_flags_exist():
    src = open(os.path.join(ROOT, "train.py")).read()
    assert '"--obs-latency-range"' in src and '"--sensor-bias"' in src and "randomize_obs_latency" in src and "randomize_sensor_bias" in src
