"""Per-env friction and servo gains (nm_set_env_params / nm_get_env_params / nm_draw_env_params, the optional cfg.domain_rand): what needs
no device - the exports and their ctypes binding, the refusals that come before any device call, the config parsing, and the config
classes' dump, which the feature must not touch."""
import ctypes
import json
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def test_library_exports_the_three_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_set_env_params", "nm_get_env_params", "nm_draw_env_params"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d3 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 3)
    assert L.nm_set_env_params.argtypes == [vp] * 5
    assert L.nm_get_env_params.argtypes == [vp] * 5
    assert L.nm_draw_env_params.argtypes == [vp, d3, d3, vp]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_env_params\(nm_env\* env, const void\* mu_dev, const void\* p_gain_dev, const void\* kv_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_env_params\(nm_env\* env, void\* mu_dev, void\* p_gain_dev, void\* kv_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_env_params\(nm_env\* env, const double lo\[3\], const double hi\[3\], void\* stream\);", hdr)
    # what it replaces upstream (nothing), where the names come from, and whose job the value ranges of nm_set_env_params are
    assert "replaces nothing upstream" in hdr and "randomize_friction" in hdr and "friction_range" in hdr
    assert "caller's responsibility" in hdr


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_env_params", "nm_get_env_params"):
        assert getattr(L, fn)(None, None, None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env" in L.nm_last_error()
    lo, hi = (ctypes.c_double * 3)(1.0, 20.0, 0.8), (ctypes.c_double * 3)(1.0, 20.0, 0.8)
    assert L.nm_draw_env_params(None, ctypes.byref(lo), ctypes.byref(hi), None) != 0
    assert b"nm_draw_env_params" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [
    ((float("nan"), 20, 0.8), (1, 20, 0.8), b"mu must be finite"),
    ((0.5, 20, 0.8), (float("inf"), 20, 0.8), b"mu must be finite"),
    ((0.5, 20, 0.8), (1, float("nan"), 0.8), b"p_gain must be finite"),
    ((0.5, 20, float("-inf")), (1, 20, 0.8), b"kv must be finite"),
    ((1e-5, 20, 0.8), (1, 20, 0.8), b"mu must be above 1e-5"),
    ((0.0, 20, 0.8), (1, 20, 0.8), b"mu must be above 1e-5"),
    ((-0.5, 20, 0.8), (1, 20, 0.8), b"mu must be above 1e-5"),
    ((0.5, -1, 0.8), (1, 20, 0.8), b"p_gain must not be negative"),
    ((0.5, 20, -0.1), (1, 20, 0.8), b"kv must not be negative"),
    ((1.5, 20, 0.8), (1, 20, 0.8), b"lo > hi for mu"),
    ((0.5, 21, 0.8), (1, 20, 0.8), b"lo > hi for p_gain"),
    ((0.5, 20, 0.9), (1, 20, 0.8), b"lo > hi for kv"),
])
def test_draw_refuses_bad_bounds_before_it_looks_at_the_device(L, lo, hi, word):
    """The bounds are judged before the handle: without any env (and without a GPU) a bad range is named, a good one gets as far as the
    missing handle."""
    l, h = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*hi)
    assert L.nm_draw_env_params(None, ctypes.byref(l), ctypes.byref(h), None) != 0
    assert word in L.nm_last_error(), L.nm_last_error()
    assert L.nm_draw_env_params(None, None, None, None) != 0 and b"lo / hi is NULL" in L.nm_last_error()


def _cfg(**kw):
    dr = types.SimpleNamespace(**kw) if kw else None
    return types.SimpleNamespace(**({"domain_rand": dr} if dr is not None else {}))


def test_optional_domain_rand_is_parsed_into_ranges():
    from nightmare_rl_amd.envs.nightmare_v3_env import env_param_config as f
    assert f(_cfg()) == (None, None, None)
    assert f(_cfg(push_robots=True, push_interval_s=1.0, max_push_vel_xy=1.0)) == (None, None, None)          # pushes alone
    assert f(_cfg(randomize_friction=False, friction_range=[0.5, 1.25])) == (None, None, None)
    assert f(_cfg(randomize_friction=True, friction_range=[0.5, 1.25])) == ((0.5, 1.25), None, None)
    assert f(_cfg(randomize_gains=True, stiffness_multiplier_range=(0.9, 1.1), damping_multiplier_range=(0.8, 1.2))) == (None, (0.9, 1.1), (0.8, 1.2))
    assert f(_cfg(randomize_gains=True, stiffness_multiplier_range=(0.9, 1.1))) == (None, (0.9, 1.1), None)
    assert f(_cfg(randomize_friction=True, friction_range=(1.0, 1.0), randomize_gains=True, damping_multiplier_range=(0.0, 2.0))) == ((1.0, 1.0), None, (0.0, 2.0))
    with pytest.raises(ValueError, match="friction_range"):
        f(_cfg(randomize_friction=True))
    with pytest.raises(ValueError, match="randomize_gains"):
        f(_cfg(randomize_gains=True))
    for bad in ([1.0, 0.5], [0.0, 1.0], [1e-5, 1.0], [-1.0, 1.0], [0.5, float("inf")], [float("nan"), 1.0], [0.5], 0.7, [0.5, 1.0, 1.5]):
        with pytest.raises(ValueError, match="friction_range"):
            f(_cfg(randomize_friction=True, friction_range=bad))
    for bad in ([1.1, 0.9], [-0.1, 1.0], [0.5, float("nan")]):
        with pytest.raises(ValueError, match="stiffness_multiplier_range"):
            f(_cfg(randomize_gains=True, stiffness_multiplier_range=bad))
        with pytest.raises(ValueError, match="damping_multiplier_range"):
            f(_cfg(randomize_gains=True, damping_multiplier_range=bad))


def test_a_user_subclass_adds_the_ranges_and_the_shipped_config_does_not_have_them():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import env_param_config, push_config

    class RandomisedConfig(NightmareV3Config):
        class domain_rand:
            randomize_friction, friction_range = True, [0.5, 1.25]
            randomize_gains, stiffness_multiplier_range, damping_multiplier_range = True, [0.9, 1.1], [0.9, 1.1]

    assert env_param_config(RandomisedConfig()) == ((0.5, 1.25), (0.9, 1.1), (0.9, 1.1))
    assert push_config(RandomisedConfig(), 0.016) == (0, 0.0)           # the class need not carry the push fields
    assert not hasattr(NightmareV3Config, "domain_rand") and env_param_config(NightmareV3Config()) == (None, None, None)


def test_command_line_flags_exist():
    for path in ("train.py", os.path.join("scripts", "play.py")):
        src = open(os.path.join(ROOT, path)).read()
        assert '"--friction-range"' in src and '"--gain-range"' in src, path


def test_config_classes_still_dump_exactly_the_golden_tree():
    """class_to_dict of the shipped config classes against tests/golden/config_class_to_dict.json, as test_abi_and_host.py compares them
    (that test remains the yardstick): the feature adds no attribute to the pinned tree."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    ours = {"NightmareV3Config": class_to_dict(NightmareV3Config()), "NightmareV3ConfigPPO": class_to_dict(NightmareV3ConfigPPO())}
    assert "domain_rand" not in ours["NightmareV3Config"] and "domain_rand" not in ref["NightmareV3Config"]
    assert ours["NightmareV3Config"].pop("device") == "cuda" and ref["NightmareV3Config"].pop("device") == "cpu"
    assert ours["NightmareV3Config"]["viewer"] == {"record_states": False, "render": False}
    ours["NightmareV3Config"]["viewer"] = ref["NightmareV3Config"]["viewer"]
    _same(ours, ref)


def _same(a, b, path=""):
    assert type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))), (path, a, b)
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same(a[k], b[k], path + "." + k)
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)
    return True
