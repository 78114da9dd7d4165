"""Push perturbations (nm_set_push / nm_get_push, the optional cfg.domain_rand): what needs no device - the exports and their ctypes binding,
the refusals that come before any device call, the seconds -> steps conversion, and the config classes' dump, which the feature must not
touch."""
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


def test_library_exports_the_push_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_set_push", "nm_get_push"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp = ctypes.c_void_p
    assert L.nm_set_push.argtypes == [vp, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64]
    assert L.nm_get_push.argtypes == [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_push\(nm_env\* env, int32_t interval_steps, double max_vel_xy, uint64_t start_step\);", hdr)
    assert re.search(r"int nm_get_push\(nm_env\* env, int32_t\* interval_steps, double\* max_vel_xy, uint64_t\* step\);", hdr)
    assert "SURVEY 8(f) row 4" in hdr and "the reference has no such line" in hdr


def test_a_null_handle_is_refused_by_name(L):
    assert L.nm_set_push(None, 3, 0.5, 0) != 0
    assert b"nm_set_push" in L.nm_last_error() and b"env" in L.nm_last_error()
    iv, mx, st = ctypes.c_int32(7), ctypes.c_double(7), ctypes.c_uint64(7)
    assert L.nm_get_push(None, ctypes.byref(iv), ctypes.byref(mx), ctypes.byref(st)) != 0
    assert b"nm_get_push" in L.nm_last_error() and b"env" in L.nm_last_error()
    assert (iv.value, mx.value, st.value) == (7, 7.0, 7)


def _cfg(**kw):
    dr = types.SimpleNamespace(**kw) if kw else None
    return types.SimpleNamespace(**({"domain_rand": dr} if dr is not None else {}))


def test_optional_domain_rand_is_parsed_into_steps():
    from nightmare_rl_amd.envs.nightmare_v3_env import push_config
    dt = 0.008 * 2
    assert push_config(_cfg(), dt) == (0, 0.0)                                                          # no class at all
    assert push_config(_cfg(push_robots=False, push_interval_s=15, max_push_vel_xy=1.0), dt) == (0, 0.0)
    assert push_config(_cfg(push_robots=True, push_interval_s=15, max_push_vel_xy=1.0), dt) == (937, 1.0)   # 15 / 0.016 = 937.5
    assert push_config(_cfg(push_robots=True, push_interval_s=0.048, max_push_vel_xy=0.5), dt) == (3, 0.5)  # 2.9999999999999996 in doubles
    assert push_config(_cfg(push_robots=True, push_interval_s=0.016, max_push_vel_xy=0.0), dt) == (1, 0.0)
    with pytest.raises(ValueError, match="push_interval_s"):
        push_config(_cfg(push_robots=True, push_interval_s=0.015, max_push_vel_xy=1.0), dt)              # below one step
    with pytest.raises(ValueError, match="push_interval_s"):
        push_config(_cfg(push_robots=True, push_interval_s=0.016, max_push_vel_xy=1.0), 0.008 * 4)      # one step of another decimation
    with pytest.raises(ValueError, match="push_interval_s"):
        push_config(_cfg(push_robots=True, push_interval_s=float("nan"), max_push_vel_xy=1.0), dt)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_push_vel_xy"):
            push_config(_cfg(push_robots=True, push_interval_s=1.0, max_push_vel_xy=bad), dt)


def test_a_user_subclass_adds_domain_rand_and_the_shipped_config_does_not_have_it():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import push_config

    class PushedConfig(NightmareV3Config):
        class domain_rand:
            push_robots, push_interval_s, max_push_vel_xy = True, 8.0, 0.75

    assert push_config(PushedConfig(), 0.016) == (500, 0.75)
    assert not hasattr(NightmareV3Config, "domain_rand") and push_config(NightmareV3Config(), 0.016) == (0, 0.0)


def test_config_classes_still_dump_exactly_the_golden_tree():
    """class_to_dict of the shipped config classes against tests/golden/config_class_to_dict.json, as test_abi_and_host.py compares them
    (that test remains the yardstick): the feature adds no attribute to the pinned tree."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    ours = {"NightmareV3Config": class_to_dict(NightmareV3Config()), "NightmareV3ConfigPPO": class_to_dict(NightmareV3ConfigPPO())}
    assert "domain_rand" not in ours["NightmareV3Config"] and "domain_rand" not in ref["NightmareV3Config"]
    # the three defaults this backend changes on purpose
    assert ours["NightmareV3Config"].pop("device") == "cuda" and ref["NightmareV3Config"].pop("device") == "cpu"
    assert ours["NightmareV3Config"]["viewer"] == {"record_states": False, "render": False}
    ours["NightmareV3Config"]["viewer"] = ref["NightmareV3Config"]["viewer"]

    def same(a, b, path=""):
        assert type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))), (path, a, b)
        if isinstance(a, dict):
            assert list(a) == list(b), (path, list(a), list(b))
            for k in a:
                same(a[k], b[k], path + "." + k)
        elif isinstance(a, list):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{path}[{i}]")
        else:
            assert a == b, (path, a, b)

    same(ours, ref)
