"""The servo target model (nm_set_servo / nm_get_servo / nm_draw_servo / nm_get_servo_state / nm_set_servo_state, the optional
cfg.control.action_rate_limit / d_gain and cfg.domain_rand ranges): what needs no device - the config parsing with every ValueError, that
the shipped config tree is unchanged, the exports with their ctypes binding and header text, the refusals that come before the handle is
looked at, and the numpy restatement of the draw over oracle.rand_u24 that tests/test_gpu_servo.py holds the device against. (The
admission of rows is the host's nmrows::servo_rows_fault: tests/test_servo_emulated.py drives it through the emulation shim.)"""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 2 ** 64 - 1
INF = float("inf")


def servo_key():
    """nm::kServoKey as nm_core.h states it."""
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_core.h")).read()
    return int(re.search(r"kServoKey = (0x[0-9A-Fa-f]+)ull", src).group(1), 16)


def draw_restated(seed, env_ids, lo, hi, npdt):
    """[n,2] (rate, d_gain) as nm_draw_servo writes them: value = lo + u (hi - lo) in the env's precision, product and sum rounded
    separately, u = rand_u24(seed + kServoKey, global env id, column) (24 bits: exact in either precision)."""
    from oracle import oracle as orc
    lo, hi = np.asarray(lo, np.float64).astype(npdt), np.asarray(hi, np.float64).astype(npdt)
    out = np.empty((len(env_ids), 2), npdt)
    for c in range(2):
        u = np.array([orc.rand_u24((seed + servo_key()) & MASK, int(e), c) for e in env_ids]).astype(npdt)
        w = hi[c] - lo[c]
        p = u * w
        out[:, c] = lo[c] + p
    assert out.dtype == npdt
    return out


def limiter_restated(lim, target, rate):
    """One step of the limiter in the dtype of its arguments: d = T - L; L' = |d| <= rate ? T : L + copysign(rate, d)."""
    d = target - lim
    return np.where(np.abs(d) <= rate, target, lim + np.copysign(rate, d)).astype(lim.dtype)


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(control=None, **kw):
    return types.SimpleNamespace(control=types.SimpleNamespace(**(control or {})), domain_rand=types.SimpleNamespace(**kw))


def test_upstreams_own_names_and_the_optional_ranges_are_parsed():
    from nightmare_rl_amd.envs.nightmare_v3_env import servo_config as f
    assert f(types.SimpleNamespace()) == (None, None)
    assert f(_cfg()) == (None, None)
    assert f(_cfg(dict(action_rate_limit=0.08))) == ((0.08, 0.08), None)
    assert f(_cfg(dict(d_gain=0.05))) == (None, (0.05, 0.05))
    assert f(_cfg(dict(d_gain=0.05, action_rate_limit=0.08))) == ((0.08, 0.08), (0.05, 0.05))      # reference config :37-38, un-commented
    assert f(_cfg(dict(action_rate_limit=INF))) == (None, None)      # inf = no limit
    assert f(_cfg(dict(d_gain=0))) == (None, (0.0, 0.0))
    assert f(_cfg(randomize_action_rate_limit=False, action_rate_limit_range=[0.02, 0.1])) == (None, None)
    assert f(_cfg(randomize_action_rate_limit=True, action_rate_limit_range=[0.02, 0.1])) == ((0.02, 0.1), None)
    assert f(_cfg(randomize_d_gain=True, d_gain_range=(0, 0.2))) == (None, (0.0, 0.2))
    # a range takes the place of the value of cfg.control
    assert f(_cfg(dict(action_rate_limit=0.08, d_gain=0.05), randomize_d_gain=True, d_gain_range=(0.0, 0.1))) == ((0.08, 0.08), (0.0, 0.1))
    assert f(_cfg(dict(action_rate_limit=0.08), randomize_action_rate_limit=True, action_rate_limit_range=(0.04, 0.1))) == ((0.04, 0.1), None)


def test_every_value_error_of_the_config():
    from nightmare_rl_amd.envs.nightmare_v3_env import servo_config as f
    for bad in (0, -0.1, float("nan"), "fast", [0.1]):
        with pytest.raises(ValueError, match="action_rate_limit"):
            f(_cfg(dict(action_rate_limit=bad)))
    for bad in (-0.01, INF, float("nan"), "stiff", [0.1]):
        with pytest.raises(ValueError, match="d_gain"):
            f(_cfg(dict(d_gain=bad)))
    with pytest.raises(ValueError, match="randomize_action_rate_limit needs action_rate_limit_range"):
        f(_cfg(randomize_action_rate_limit=True))
    with pytest.raises(ValueError, match="randomize_d_gain needs d_gain_range"):
        f(_cfg(randomize_d_gain=True))
    for bad in ([1.0, 0.5], [float("nan"), 1.0], [0.1, INF], 3.0, [1.0, 2.0, 3.0], "ab"):
        with pytest.raises(ValueError, match="action_rate_limit_range"):
            f(_cfg(randomize_action_rate_limit=True, action_rate_limit_range=bad))
        with pytest.raises(ValueError, match="d_gain_range"):
            f(_cfg(randomize_d_gain=True, d_gain_range=bad))
    for bad in ([0.0, 0.1], [-0.1, 0.1]):      # 0 < lo
        with pytest.raises(ValueError, match="action_rate_limit_range"):
            f(_cfg(randomize_action_rate_limit=True, action_rate_limit_range=bad))
    with pytest.raises(ValueError, match="d_gain_range"):      # 0 <= lo
        f(_cfg(randomize_d_gain=True, d_gain_range=[-0.1, 0.1]))


def test_the_shipped_config_tree_is_unchanged_and_a_user_adds_the_two_lines():
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import servo_config
    cfg = NightmareV3Config()
    assert not hasattr(cfg.control, "action_rate_limit") and not hasattr(cfg.control, "d_gain") and not hasattr(cfg, "domain_rand")
    assert servo_config(cfg) == (None, None)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    assert "action_rate_limit" not in json.dumps(golden) and "d_gain" not in json.dumps(golden)
    assert sorted(class_to_dict(cfg.control)) == ["action_scale", "decimation", "default_pos", "p_gain"]
    cfg.control.d_gain, cfg.control.action_rate_limit = 0.05, 0.08      # what un-commenting reference config :37-38 does
    assert servo_config(cfg) == ((0.08, 0.08), (0.05, 0.05))


def test_the_command_line_flags_exist():
    for script in ("train.py", os.path.join("scripts", "play.py")):
        src = open(os.path.join(ROOT, script)).read()
        assert '"--action-rate-limit"' in src and '"--d-gain"' in src
        assert "cfg.control.action_rate_limit = " in src and "cfg.control.d_gain = " in src


# ---------------------------------------------------------------------------------------------------------------- the restatements
def test_the_restated_draw_is_keyed_by_the_global_env_id():
    """What the device is held against (tests/test_gpu_servo.py): in range, not constant, and shards draw what the whole draws."""
    assert servo_key() == int.from_bytes(b"SERVO", "big")
    lo, hi = [0.02, 0.0], [0.1, 0.2]
    for npdt in (np.float32, np.float64):
        whole = draw_restated(5, np.arange(100, 164), lo, hi, npdt)
        parts = np.concatenate([draw_restated(5, np.arange(100, 132), lo, hi, npdt), draw_restated(5, np.arange(132, 164), lo, hi, npdt)])
        np.testing.assert_array_equal(whole, parts)
        for c in range(2):
            assert whole[:, c].min() >= npdt(lo[c]) and whole[:, c].max() <= npdt(hi[c]) and np.unique(whole[:, c]).size > 50
        assert not np.array_equal(whole[:, 0], whole[:, 1])
        np.testing.assert_array_equal(draw_restated(5, np.arange(8, 16), lo, hi, npdt), draw_restated(5, np.arange(16), lo, hi, npdt)[8:])
    np.testing.assert_array_equal(draw_restated(5, [7], [0.05, 0.1], [0.05, 0.1], np.float32), np.array([[0.05, 0.1]], np.float32))      # lo == hi pins a column


def test_the_restated_limiter_reproduces_the_fixture():
    """The recursion the GPU test holds servo_state() against, on the reference's own recorded targets (fp64): bit for bit."""
    from conftest import load_golden
    G = load_golden("servo.npz")
    dp = np.tile([0.0, np.pi / 5, 0.0], 6)
    for rec, delays in (("S", np.zeros(8, int)), ("SL", G["delays"])):
        k = delays // 2
        for pop in ("drop", "stand"):
            lim, hist, act = G[f"{rec}_{pop}_lim"], G[f"{rec}_{pop}_hist"], G[f"{rec}_{pop}_act"]
            for t in range(lim.shape[0] - 1):
                late = np.stack([act[t + 1][e] if k[e] == 0 else hist[t][e, k[e] - 1].astype(np.float64) for e in range(8)])
                np.testing.assert_array_equal(limiter_restated(lim[t], late - dp, G["rate"][:, None]), lim[t + 1])
    assert limiter_restated(np.float32([0.0, 0.0, 0.5]), np.float32([0.3, -0.3, 0.52]), np.float32(0.08)).tolist() == [np.float32(0.08), np.float32(-0.08), np.float32(0.52)]
    assert limiter_restated(np.float64([0.25]), np.float64([-7.0]), np.inf)[0] == -7.0      # +inf: the target itself


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
    for name in ("nm_set_servo", "nm_get_servo", "nm_draw_servo", "nm_get_servo_state", "nm_set_servo_state"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d2 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 2)
    assert L.nm_set_servo.argtypes == [vp] * 3
    assert L.nm_get_servo.argtypes == [vp] * 3
    assert L.nm_draw_servo.argtypes == [vp, d2, d2, vp]
    assert L.nm_get_servo_state.argtypes == [vp] * 2 and L.nm_set_servo_state.argtypes == [vp] * 2
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_servo\(nm_env\* env, const void\* rows_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_servo\(nm_env\* env, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_servo\(nm_env\* env, const double lo\[2\], const double hi\[2\], void\* stream\);", hdr)
    assert re.search(r"int nm_get_servo_state\(nm_env\* env, double\* limited\);", hdr)
    assert re.search(r"int nm_set_servo_state\(nm_env\* env, const double\* limited\);", hdr)
    # the header cites the reference lines it replaces and says what a non-finite buffer does
    for words in ("envs/nightmare_v3_env.py:97", "envs/nightmare_v3_env.py:187-188", "envs/nightmare_v3_config.py:37-38", "L + copysign(rate, d)",
                  "non-finite dof_vel", "limited_actions"):
        assert words in hdr, words


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_servo", "nm_get_servo"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    for fn in ("nm_get_servo_state", "nm_set_servo_state"):
        assert getattr(L, fn)(None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    lo, hi = (ctypes.c_double * 2)(0.02, 0.0), (ctypes.c_double * 2)(0.1, 0.2)
    assert L.nm_draw_servo(None, ctypes.byref(lo), ctypes.byref(hi), None) != 0
    assert b"nm_draw_servo" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert L.nm_draw_servo(None, None, ctypes.byref(hi), None) != 0 and b"lo / hi is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [
    ((float("nan"), 0), (1, 0), b"rate must be finite"),
    ((0.1, 0), (INF, 0), b"rate must be finite"),
    ((0.1, 0), (0.2, INF), b"d_gain must be finite"),
    ((0.5, 0), (0.1, 0), b"lo > hi for rate"),
    ((0.1, 0.2), (0.1, 0.1), b"lo > hi for d_gain"),
    ((0.0, 0), (0.1, 0), b"rate must be above 0"),
    ((-0.1, 0), (0.1, 0), b"rate must be above 0"),
    ((0.1, -0.1), (0.1, 0.1), b"d_gain must not be negative"),
])
def test_bad_ranges_are_refused_before_the_handle_is_looked_at(L, lo, hi, word):
    a, b = (ctypes.c_double * 2)(*lo), (ctypes.c_double * 2)(*hi)
    assert L.nm_draw_servo(None, ctypes.byref(a), ctypes.byref(b), None) != 0
    assert word in L.nm_last_error(), L.nm_last_error()
