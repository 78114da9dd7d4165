"""The servo torque limit (nm_set_torque_limit / nm_get_torque_limit / nm_draw_torque_limit, the optional cfg.control.torque_limit and
cfg.domain_rand.randomize_torque_limit / torque_limit_range): what needs no device - the config parsing with every ValueError, that the
shipped config tree is unchanged, the exports with their ctypes binding and header text, the refusals that come before the handle is
looked at, the numpy restatement of the draw over oracle.rand_u24 that tests/test_gpu_torque_limit.py holds the device against, and the
numpy clamp and mask on the fixture's own end-of-step forces. (The admission of rows is the host's nmrows::torque_rows_fault:
tests/test_torque_limit_emulated.py drives it through the emulation shim.)"""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

from torque_tools import POPS, clamp_and_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 2 ** 64 - 1
INF = float("inf")


def torque_key():
    """nm::kTorqueKey as nm_core.h states it."""
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_core.h")).read()
    return int(re.search(r"kTorqueKey = (0x[0-9A-Fa-f]+)ull", src).group(1), 16)


def draw_restated(seed, env_ids, lo, hi, npdt):
    """[n,3] limits as nm_draw_torque_limit writes them: value = lo + u (hi - lo) in the env's precision, product and sum rounded
    separately, u = rand_u24(seed + kTorqueKey, global env id, column) (24 bits: exact in either precision)."""
    from oracle import oracle as orc
    lo, hi = np.asarray(lo, np.float64).astype(npdt), np.asarray(hi, np.float64).astype(npdt)
    out = np.empty((len(env_ids), 3), npdt)
    for c in range(3):
        u = np.array([orc.rand_u24((seed + torque_key()) & MASK, int(e), c) for e in env_ids]).astype(npdt)
        w = hi[c] - lo[c]
        p = u * w
        out[:, c] = lo[c] + p
    assert out.dtype == npdt
    return out


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(control=None, **kw):
    return types.SimpleNamespace(control=types.SimpleNamespace(**(control or {})), domain_rand=types.SimpleNamespace(**kw))


def test_the_config_names_are_parsed():
    from nightmare_rl_amd.envs.nightmare_v3_env import torque_config as f
    assert f(types.SimpleNamespace()) == (None, None)
    assert f(_cfg()) == (None, None)
    assert f(_cfg(dict(torque_limit=3.2))) == ([3.2, 3.2, 3.2], None)
    assert f(_cfg(dict(torque_limit=[6.4, 0.3, 2.4]))) == ([6.4, 0.3, 2.4], None)
    assert f(_cfg(dict(torque_limit=(INF, 1.6, INF)))) == ([INF, 1.6, INF], None)
    assert f(_cfg(randomize_torque_limit=False, torque_limit_range=[2.0, 4.0])) == (None, None)
    assert f(_cfg(randomize_torque_limit=True, torque_limit_range=[2.0, 4.0])) == (None, [[2.0, 4.0]] * 3)
    assert f(_cfg(randomize_torque_limit=True, torque_limit_range=[[2, 4], [1, 1], [3, 5]])) == (None, [[2.0, 4.0], [1.0, 1.0], [3.0, 5.0]])
    assert f(_cfg(dict(torque_limit=3.2), randomize_torque_limit=True, torque_limit_range=(2.0, 4.0))) == ([3.2] * 3, [[2.0, 4.0]] * 3)


def test_every_value_error_of_the_config():
    from nightmare_rl_amd.envs.nightmare_v3_env import torque_config as f
    for bad in (0, -1.0, float("nan"), "strong", [1.0, 2.0], [1.0, 2.0, 0.0], [1.0, 2.0, 3.0, 4.0]):
        with pytest.raises(ValueError, match="torque_limit"):
            f(_cfg(dict(torque_limit=bad)))
    with pytest.raises(ValueError, match="randomize_torque_limit needs torque_limit_range"):
        f(_cfg(randomize_torque_limit=True))
    for bad in ([1.0, 0.5], [float("nan"), 1.0], [0.1, INF], 3.0, [1.0, 2.0, 3.0], "ab", [0.0, 1.0], [-1.0, 1.0], [[1, 2], [1, 2]], [[1, 2], [1, 2], [2, 1]]):
        with pytest.raises(ValueError, match="torque_limit_range"):
            f(_cfg(randomize_torque_limit=True, torque_limit_range=bad))


def test_the_shipped_config_tree_is_unchanged():
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import torque_config
    cfg = NightmareV3Config()
    assert not hasattr(cfg.control, "torque_limit") and not hasattr(cfg, "domain_rand")
    assert torque_config(cfg) == (None, None)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    assert "torque_limit" not in json.dumps(golden)
    assert sorted(class_to_dict(cfg.control)) == ["action_scale", "decimation", "default_pos", "p_gain"]
    cfg.control.torque_limit = 3.2
    assert torque_config(cfg) == ([3.2, 3.2, 3.2], None)


def test_the_command_line_flag_exists():
    for script in ("train.py", os.path.join("scripts", "play.py")):
        src = open(os.path.join(ROOT, script)).read()
        assert '"--torque-limit"' in src and "cfg.control.torque_limit = " in src


# ---------------------------------------------------------------------------------------------------------------- the restatements
def test_the_restated_draw_is_keyed_by_the_global_env_id():
    """What the device is held against (tests/test_gpu_torque_limit.py): in range, not constant, three independent columns, and a shard
    with env_offset = 8 draws the slice [8:16] of a 16-env draw."""
    assert torque_key() == int.from_bytes(b"TORQUE", "big")
    lo, hi = [2.0, 0.5, 1.0], [4.0, 0.5, 3.0]
    for npdt in (np.float32, np.float64):
        whole = draw_restated(5, np.arange(100, 164), lo, hi, npdt)
        for c in (0, 2):
            assert whole[:, c].min() >= npdt(lo[c]) and whole[:, c].max() <= npdt(hi[c]) and np.unique(whole[:, c]).size > 50
        assert (whole[:, 1] == npdt(0.5)).all()      # lo == hi pins a column
        u0, u2 = (whole[:, 0] - npdt(2.0)) / npdt(2.0), (whole[:, 2] - npdt(1.0)) / npdt(2.0)
        assert np.abs(u0 - u2).max() > 0.5      # independent draws, not one draw scaled three times
        np.testing.assert_array_equal(draw_restated(5, np.arange(8, 16), lo, hi, npdt), draw_restated(5, np.arange(16), lo, hi, npdt)[8:])


def test_the_numpy_clamp_and_mask_reproduce_the_fixtures_forces():
    """On the reference's own end-of-step qfrc_actuator: the clamp is idempotent on a recorded force, a recorded force never exceeds its
    bound, the mask is 0 exactly on the saturated joint-steps and 1 elsewhere, and the semantics' corner cases."""
    from conftest import load_golden
    G = load_golden("torque.npz")
    for pop in POPS:
        for k, fmax in enumerate(G["sets"]):
            f = G[f"{pop}_qfrc"][k]
            fc, d = clamp_and_mask(f, fmax)
            np.testing.assert_array_equal(fc, f)
            lim = np.tile(fmax, 6)
            assert (np.abs(f) <= lim).all()
            np.testing.assert_array_equal(d == 0, np.abs(f) == lim)
            if k == 0:
                assert d.all()
    # word k limits joint 3 leg + k; the range is symmetric; the bound itself is saturated; +inf never clamps; NaN stays NaN and is masked out
    f = np.array([5.0, -5.0, 0.2, 3.2, -0.3, np.nan] + [0.0] * 12)
    fc, d = clamp_and_mask(f, [3.2, 0.3, INF])
    assert fc[:5].tolist() == [3.2, -0.3, 0.2, 3.2, -0.3] and np.isnan(fc[5])
    assert d[:6].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


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
    for name in ("nm_set_torque_limit", "nm_get_torque_limit", "nm_draw_torque_limit"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d3 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 3)
    assert L.nm_set_torque_limit.argtypes == [vp] * 3
    assert L.nm_get_torque_limit.argtypes == [vp] * 3
    assert L.nm_draw_torque_limit.argtypes == [vp, d3, d3, vp]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_torque_limit\(nm_env\* env, const void\* rows_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_torque_limit\(nm_env\* env, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_torque_limit\(nm_env\* env, const double lo\[3\], const double hi\[3\], void\* stream\);", hdr)
    # the header cites the MuJoCo stages the entry points stand for and states the clamp as selects
    for words in ("forcerange", "mj_fwdActuation", "mjd_actuator_vel", "mj_implicit", "f > fmax ? fmax : (f < -fmax ? -fmax : f)", "M + h kv D",
                  "a NaN force stays NaN", '"TORQUE"'):
        assert words in hdr, words


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_torque_limit", "nm_get_torque_limit"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    lo, hi = (ctypes.c_double * 3)(1.0, 1.0, 1.0), (ctypes.c_double * 3)(2.0, 2.0, 2.0)
    assert L.nm_draw_torque_limit(None, ctypes.byref(lo), ctypes.byref(hi), None) != 0
    assert b"nm_draw_torque_limit" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert L.nm_draw_torque_limit(None, None, ctypes.byref(hi), None) != 0 and b"lo / hi is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [
    ((float("nan"), 1, 1), (2, 2, 2), b"the coxa limit must be finite"),
    ((1, 1, 1), (2, INF, 2), b"the femur limit must be finite"),
    ((1, 1, 3), (2, 2, 2), b"lo > hi for the tibia limit"),
    ((0.0, 1, 1), (2, 2, 2), b"a limit must be above 0"),
    ((1, -0.5, 1), (2, 2, 2), b"a limit must be above 0"),
])
def test_bad_ranges_are_refused_before_the_handle_is_looked_at(L, lo, hi, word):
    a, b = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*hi)
    assert L.nm_draw_torque_limit(None, ctypes.byref(a), ctypes.byref(b), None) != 0
    assert word in L.nm_last_error(), L.nm_last_error()
