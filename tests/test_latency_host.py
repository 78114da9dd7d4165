"""Per-env actuation latency (nm_set_action_latency / nm_get_action_latency / nm_draw_action_latency / nm_set_action_history /
nm_get_action_history, the optional cfg.domain_rand): what needs no device - the exports and their ctypes binding, the refusals that come
before any device call, the config parsing, the config classes' dump, which the feature must not touch, and the numpy restatement of the
draw that the GPU test holds the device against."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENCY_KEY = 0x4C4154454E       # nm_core.h kLatencyKey ("LATEN")
NAMES = ("nm_set_action_latency", "nm_get_action_latency", "nm_draw_action_latency", "nm_set_action_history", "nm_get_action_history")


def draw_np(seed, env_offset, n, lo, hi):
    """nm_draw_action_latency restated: delay[e] = lo + floor(u (hi - lo + 1)), u = rand_u24(seed + kLatencyKey, global env id, 0) - 24
    bits times 2^-24, so the product with a small integer is exact in float64 and the floor is the device's integer shift."""
    from oracle import oracle as orc
    u = np.array([orc.rand_u24((seed + LATENCY_KEY) & (2 ** 64 - 1), env_offset + e, 0) for e in range(n)], np.float64)
    assert ((u * 2 ** 24) == np.round(u * 2 ** 24)).all() and (u >= 0).all() and (u < 1).all()
    return (lo + np.floor(u * (hi - lo + 1))).astype(np.int32)


def test_the_restated_draw_is_uniform_on_the_closed_integer_range():
    d = draw_np(7, 0, 7000, 0, 6)
    assert d.min() == 0 and d.max() == 6
    counts = np.bincount(d, minlength=7)
    print("counts of delays 0..6 over 7000 envs:", counts.tolist())
    # 7 equally likely values, 1000 expected each, sigma = sqrt(7000 * 1/7 * 6/7) = 29.3: six sigma
    assert (np.abs(counts - 1000) < 176).all()
    np.testing.assert_array_equal(draw_np(7, 0, 64, 3, 3), np.full(64, 3))
    d25 = draw_np(7, 0, 512, 2, 5)
    assert d25.min() == 2 and d25.max() == 5
    # keyed by the global env id: a shard draws what its envs got in the whole population
    np.testing.assert_array_equal(draw_np(7, 8, 8, 0, 6), draw_np(7, 0, 16, 0, 6)[8:])


# ---------------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def test_library_exports_the_five_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert L.nm_set_action_latency.argtypes == [vp] * 3
    assert L.nm_get_action_latency.argtypes == [vp] * 3
    assert L.nm_draw_action_latency.argtypes == [vp, i32, i32, vp]
    assert L.nm_set_action_history.argtypes == [vp] * 3
    assert L.nm_get_action_history.argtypes == [vp] * 3
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_action_latency\(nm_env\* env, const int32_t\* substeps_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_action_latency\(nm_env\* env, int32_t\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_action_latency\(nm_env\* env, int32_t lo, int32_t hi, void\* stream\);", hdr)
    assert re.search(r"int nm_set_action_history\(nm_env\* env, const float\* hist_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_action_history\(nm_env\* env, float\* out_dev, void\* stream\);", hdr)
    # the semantics, and that there is no upstream line
    assert "There is no reference line" in hdr and "a_{t-k-1} while s < r and at a_{t-k} from s = r on" in hdr
    assert "hist[e][j] = a_{t-1-j}" in hdr and "physics-only launches (which ignore latency altogether)" in hdr


def test_the_key_in_the_kernel_source_is_the_tests_key():
    src = open(os.path.join(ROOT, "nightmare_rl_amd", "csrc", "nm_core.h")).read()
    m = re.search(r"kLatencyKey = (0x[0-9A-Fa-f]+)ull", src)
    assert m and int(m.group(1), 16) == LATENCY_KEY and LATENCY_KEY.to_bytes(5, "big") == b"LATEN"
    assert re.search(r"constexpr int kLatH = 3\b", src)


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_action_latency", "nm_get_action_latency", "nm_set_action_history", "nm_get_action_history"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    assert L.nm_draw_action_latency(None, 0, 6, None) != 0
    assert b"nm_draw_action_latency" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [(-1, 3, b"lo < 0"), (4, 3, b"lo > hi"), (-2, -3, b"lo < 0")])
def test_bad_ranges_are_refused_before_the_handle_is_looked_at(L, lo, hi, word):
    assert L.nm_draw_action_latency(None, lo, hi, None) != 0
    assert word in L.nm_last_error() and b"env is NULL" not in L.nm_last_error(), L.nm_last_error()


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(**kw):
    return types.SimpleNamespace(domain_rand=types.SimpleNamespace(**kw))


def test_optional_domain_rand_is_parsed_into_a_range():
    from nightmare_rl_amd.envs.nightmare_v3_env import latency_config as f
    assert f(types.SimpleNamespace()) is None
    assert f(_cfg(randomize_action_latency=False, action_latency_range=[0, 6])) is None
    assert f(_cfg(randomize_action_latency=True, action_latency_range=[0, 6])) == (0, 6)
    assert f(_cfg(randomize_action_latency=True, action_latency_range=(2.0, 2.0))) == (2, 2)
    with pytest.raises(ValueError, match="needs action_latency_range"):
        f(_cfg(randomize_action_latency=True))
    for bad in ([3, 1], [-1, 2], [0.5, 2], [0, float("inf")], [float("nan"), 1], 3, [1, 2, 3]):
        with pytest.raises(ValueError, match="action_latency_range"):
            f(_cfg(randomize_action_latency=True, action_latency_range=bad))


def test_a_user_subclass_adds_the_range_and_the_shipped_config_does_not_have_it():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import env_param_config, latency_config, payload_config, push_config

    class RandomisedConfig(NightmareV3Config):
        class domain_rand:
            randomize_action_latency, action_latency_range = True, [1, 4]

    assert latency_config(RandomisedConfig()) == (1, 4)
    assert push_config(RandomisedConfig(), 0.016) == (0, 0.0) and env_param_config(RandomisedConfig()) == (None, None, None)
    assert payload_config(RandomisedConfig()) == (None, None)
    assert not hasattr(NightmareV3Config, "domain_rand") and latency_config(NightmareV3Config()) is None


def test_command_line_flags_exist():
    for path in ("train.py", os.path.join("scripts", "play.py")):
        src = open(os.path.join(ROOT, path)).read()
        assert '"--latency-range"' in src and "action_latency_range" in src, path


def test_config_classes_still_dump_exactly_the_golden_tree():
    """class_to_dict of the shipped config classes against tests/golden/config_class_to_dict.json, as test_abi_and_host.py compares them
    (that test remains the yardstick): the feature adds no attribute to the pinned tree."""
    from test_env_params_host import _same
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    ours = {"NightmareV3Config": class_to_dict(NightmareV3Config()), "NightmareV3ConfigPPO": class_to_dict(NightmareV3ConfigPPO())}
    assert "domain_rand" not in ours["NightmareV3Config"] and "domain_rand" not in ref["NightmareV3Config"]
    assert ours["NightmareV3Config"].pop("device") == "cuda" and ref["NightmareV3Config"].pop("device") == "cpu"
    assert ours["NightmareV3Config"]["viewer"] == {"record_states": False, "render": False}
    ours["NightmareV3Config"]["viewer"] = ref["NightmareV3Config"]["viewer"]
    _same(ours, ref)
