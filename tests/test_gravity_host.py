"""Per-env gravity vectors (nm_set_gravity / nm_get_gravity / nm_draw_gravity, the optional cfg.domain_rand): what needs no device - the
config parsing with every ValueError, the float64 derivation of g from (offset, theta, phi) against a second statement, the exports and
their ctypes binding, the refusals that come before any device call, and the numpy restatement of the draw over oracle.rand_u24 that
tests/test_gpu_gravity.py holds the device against. (The admission of rows is the host's nmrows::grav_rows_fault: tests/test_gravity_emulated.py
drives it through the emulation shim.)"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 2 ** 64 - 1


def gravity_key():
    """nm::kGravityKey as nm_core.h states it."""
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_core.h")).read()
    return int(re.search(r"kGravityKey = (0x[0-9A-Fa-f]+)ull", src).group(1), 16)


def draw_restated(seed, env_ids, lo, hi, npdt):
    """[n,5] what nm_draw_gravity writes: value = lo + u (hi - lo) in the env's precision, product and sum rounded separately,
    u = rand_u24(seed + kGravityKey, global env id, column) (24 bits: exact in either precision)."""
    from oracle import oracle as orc
    lo, hi = np.asarray(lo, np.float64).astype(npdt), np.asarray(hi, np.float64).astype(npdt)
    out = np.empty((len(env_ids), 5), npdt)
    for c in range(5):
        u = np.array([orc.rand_u24((seed + gravity_key()) & MASK, int(e), c) for e in env_ids]).astype(npdt)
        w = hi[c] - lo[c]
        p = u * w
        out[:, c] = lo[c] + p
    assert out.dtype == npdt
    return out


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(**kw):
    return types.SimpleNamespace(domain_rand=types.SimpleNamespace(**kw))


def test_optional_domain_rand_is_parsed():
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_config as f
    assert f(types.SimpleNamespace()) == (None, None, True)
    assert f(_cfg(randomize_gravity=False, gravity_range=[-1.0, 1.0])) == (None, None, True)
    assert f(_cfg(randomize_gravity=True, gravity_range=[-1.0, 1.0])) == ((-1.0, 1.0), None, True)
    assert f(_cfg(randomize_slope=True, slope_range=(0.0, 0.3))) == (None, (0.0, 0.3), True)
    assert f(_cfg(randomize_slope=True, slope_range=(0.1, 0.1), randomize_gravity=True, gravity_range=(0, 0.5), gravity_observed=False)) == ((0.0, 0.5), (0.1, 0.1), False)


def test_every_value_error_of_the_config():
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_config as f
    with pytest.raises(ValueError, match="randomize_gravity needs gravity_range"):
        f(_cfg(randomize_gravity=True))
    with pytest.raises(ValueError, match="randomize_slope needs slope_range"):
        f(_cfg(randomize_slope=True))
    for bad in ([1.0, 0.5], [float("nan"), 1.0], [0.0, float("inf")], 3.0, [1.0, 2.0, 3.0], "ab"):
        with pytest.raises(ValueError, match="gravity_range"):
            f(_cfg(randomize_gravity=True, gravity_range=bad))
        with pytest.raises(ValueError, match="slope_range"):
            f(_cfg(randomize_slope=True, slope_range=bad))
    for bad in ([-0.1, 0.2], [0.0, np.pi / 2], [0.0, 2.0]):      # 0 <= lo <= hi < pi/2
        with pytest.raises(ValueError, match="slope_range"):
            f(_cfg(randomize_slope=True, slope_range=bad))
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="gravity_observed"):
            f(_cfg(gravity_observed=bad))


def test_a_user_subclass_adds_the_ranges_and_the_shipped_config_does_not_have_them():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_config, payload_config

    class SlopedConfig(NightmareV3Config):
        class domain_rand:
            randomize_gravity, gravity_range = True, [-1.0, 1.0]
            randomize_slope, slope_range = True, [0.0, 0.25]
            gravity_observed = False

    assert gravity_config(SlopedConfig()) == ((-1.0, 1.0), (0.0, 0.25), False)
    assert payload_config(SlopedConfig()) == (None, None)
    assert not hasattr(NightmareV3Config, "domain_rand") and gravity_config(NightmareV3Config()) == (None, None, True)


# ---------------------------------------------------------------------------------------------------------------- the derivation
def test_g_from_offset_tilt_and_azimuth_against_a_second_statement():
    """gravity_from_draw against rotation matrices: the nominal vector (0, 0, -9.81) rotated by -theta about y (in the frame of a floor
    that falls away towards +x gravity has the component +9.81 sin theta along x), then by phi about z, plus the offset."""
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_from_draw
    rng = np.random.default_rng(3)
    n = 64
    off, th, ph = rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 1.5, n), rng.uniform(0, 2 * np.pi, n)
    got = gravity_from_draw(off, th, ph)
    assert got.shape == (n, 3) and got.dtype == np.float64
    for i in range(n):
        Ry = np.array([[np.cos(th[i]), 0, -np.sin(th[i])], [0, 1, 0], [np.sin(th[i]), 0, np.cos(th[i])]])      # rotation by -theta about y
        Rz = np.array([[np.cos(ph[i]), -np.sin(ph[i]), 0], [np.sin(ph[i]), np.cos(ph[i]), 0], [0, 0, 1]])
        want = Rz @ Ry @ np.array([0.0, 0.0, -9.81]) + off[i]
        np.testing.assert_allclose(got[i], want, rtol=0, atol=1e-14)
        assert abs(np.linalg.norm(got[i] - off[i]) - 9.81) < 1e-13
        # the angle between g - offset and straight down is theta; its horizontal part points along the azimuth
        assert abs(np.arccos(-(got[i] - off[i])[2] / 9.81) - th[i]) < 1e-7
    np.testing.assert_array_equal(gravity_from_draw(np.zeros(3), 0.0, 0.0), [0.0, 0.0, -9.81])
    # the fixture's rows are this derivation
    from conftest import load_golden
    G = load_golden("gravity.npz")
    for s, row in zip(G["sets"], G["rows"]):
        g = gravity_from_draw(s[0:3], s[3], s[4])
        np.testing.assert_allclose(row[0:3], g, rtol=0, atol=1e-15)
        np.testing.assert_allclose(row[4:7], g if s[5] else [0, 0, -9.81], rtol=0, atol=1e-15)
        assert row[3] == 0 and row[7] == 0


def test_the_restated_draw_is_keyed_by_the_global_env_id():
    """What the device is held against (tests/test_gpu_gravity.py): in range, not constant, and shards draw what the whole draws."""
    assert gravity_key() == int.from_bytes(b"GRAV", "big")
    lo, hi = [-1.0, -1.0, -1.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.3, 2 * np.pi]
    for npdt in (np.float32, np.float64):
        whole = draw_restated(5, np.arange(100, 164), lo, hi, npdt)
        parts = np.concatenate([draw_restated(5, np.arange(100, 132), lo, hi, npdt), draw_restated(5, np.arange(132, 164), lo, hi, npdt)])
        np.testing.assert_array_equal(whole, parts)
        for c in range(5):
            assert whole[:, c].min() >= npdt(lo[c]) and whole[:, c].max() <= npdt(hi[c]) and np.unique(whole[:, c]).size > 50
        assert not np.array_equal(whole[:, 0], whole[:, 1])
    np.testing.assert_array_equal(draw_restated(5, [7], [0.5] * 5, [0.5] * 5, np.float32), np.full((1, 5), 0.5, np.float32))      # lo == hi pins a column


# ---------------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def test_library_exports_the_three_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_set_gravity", "nm_get_gravity", "nm_draw_gravity"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d5 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 5)
    assert L.nm_set_gravity.argtypes == [vp] * 3
    assert L.nm_get_gravity.argtypes == [vp] * 3
    assert L.nm_draw_gravity.argtypes == [vp, d5, d5, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_gravity\(nm_env\* env, const void\* rows_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_gravity\(nm_env\* env, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_gravity\(nm_env\* env, const double lo\[5\], const double hi\[5\], void\* out_dev, void\* stream\);", hdr)
    assert "a level floor under a gravity vector tilted by theta" in hdr and "gravity_vec" in hdr and "randomize_gravity" in hdr


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_gravity", "nm_get_gravity"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    lo, hi = (ctypes.c_double * 5)(0, 0, 0, 0, 0), (ctypes.c_double * 5)(1, 1, 1, 0.2, 6.0)
    assert L.nm_draw_gravity(None, ctypes.byref(lo), ctypes.byref(hi), None, None) != 0
    assert b"nm_draw_gravity" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert L.nm_draw_gravity(None, None, ctypes.byref(hi), None, None) != 0 and b"lo / hi is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [
    ((float("nan"), 0, 0, 0, 0), (1, 0, 0, 0, 0), b"offset x must be finite"),
    ((0, 0, 0, 0, 0), (0, float("inf"), 0, 0, 0), b"offset y must be finite"),
    ((0, 0, 0, float("-inf"), 0), (0, 0, 0, 0.1, 0), b"tilt must be finite"),
    ((0.5, 0, 0, 0, 0), (0.1, 0, 0, 0, 0), b"lo > hi for offset x"),
    ((0, 0, 0.2, 0, 0), (0, 0, 0.1, 0, 0), b"lo > hi for offset z"),
    ((0, 0, 0, 0.3, 0), (0, 0, 0, 0.2, 0), b"lo > hi for tilt"),
    ((0, 0, 0, 0, 1.0), (0, 0, 0, 0, 0.5), b"lo > hi for azimuth"),
])
def test_bad_ranges_are_refused_before_the_handle_is_looked_at(L, lo, hi, word):
    a, b = (ctypes.c_double * 5)(*lo), (ctypes.c_double * 5)(*hi)
    assert L.nm_draw_gravity(None, ctypes.byref(a), ctypes.byref(b), None, None) != 0
    assert word in L.nm_last_error(), L.nm_last_error()
