"""Per-env base payloads (nm_set_body_params / nm_get_body_params / nm_draw_payload, nightmare_rl_amd/model/payload.py, the optional
cfg.domain_rand): what needs no device - the host derivation of the body rows against the per-env path through compile_model's own
functions, its refusals, the exports and their ctypes binding, the refusals that come before any device call, the config parsing, and
the config classes' dump, which the feature must not touch."""
import ctypes
import json
import os
import re
import time
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fixture's four sets (the issue's table: meaninertia, base invweight0)
SETS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])
TABLE = np.array([[0.38196, 0.45443], [0.44456, 0.37013], [0.34446, 0.52755], [0.50741, 0.31205]])


def rel_err(row, ref):
    """Relative error of a row against the per-env path's. The six inertia words are measured against the tensor's largest moment and
    the COM against the largest coordinate: the per-env path takes I' through eigh and back (and the COM through a rotation), whose
    rounding is relative to the tensor's norm, not to each entry - the off-diagonal words are 1e-5 of the diagonal ones here."""
    scale = np.abs(ref).copy()
    scale[0:3] = np.abs(ref[0:3]).max()
    scale[3:9] = np.abs(ref[3:9]).max()
    scale[19] = 1.0
    return float((np.abs(row - ref) / scale).max())


def test_rows_equal_the_per_env_path_for_the_four_sets_and_16_random_payloads():
    from nightmare_rl_amd.model import payload
    rng = np.random.default_rng(11)
    dm = np.concatenate([SETS[:, 0], rng.uniform(0.0, 1.2, 12), rng.uniform(-0.4, 0.0, 4)])
    r = np.concatenate([SETS[:, 1:], rng.uniform(-0.06, 0.06, (12, 3)), rng.uniform(-0.01, 0.01, (4, 3))])       # a negative mass far from the COM is not admissible
    rows = payload.payload_rows(dm, r)
    assert rows.shape == (20, 20) and rows.dtype == np.float64
    worst = 0.0
    for k in range(20):
        ref = payload.row_of_tables(payload.modified_tables(dm[k], r[k]))
        worst = max(worst, rel_err(rows[k], ref))
    print("largest relative error against the per-env path:", worst)
    assert worst < 1e-12
    # the issue's table, to its five printed digits
    np.testing.assert_allclose(1.0 / (rows[:4, payload.C_PGS] * 24), TABLE[:, 0], atol=6e-6)
    np.testing.assert_allclose(rows[:4, payload.C_INVW], TABLE[:, 1], atol=6e-6)
    assert len({tuple(x) for x in np.round(rows[:4], 9)}) == 4


def test_no_payload_reproduces_the_committed_constants():
    from nightmare_rl_amd.model import compile_model as cm, payload
    T = cm.load_tables()
    row = payload.payload_rows([0.0], [[0.0, 0.0, 0.0]])[0]
    assert rel_err(row, payload.row_of_tables(T)) < 1e-12
    assert abs(row[payload.C_PGS] * T["meaninertia"] * T["nv"] - 1) < 1e-12
    np.testing.assert_allclose(row[payload.C_INVW:payload.C_INVW + 7], T["body_invweight0"][T["col_body"], 0], rtol=1e-12)
    assert row[payload.C_MASS] == T["body_mass"][1] and abs(row[payload.C_TOTAL] - 3.0) < 1e-12
    # the tibias' invweight0 moves with the base's mass: the base floats
    heavy = payload.payload_rows([1.0], [[0.0, 0.0, 0.0]])[0]
    assert (heavy[payload.C_INVW + 1:payload.C_INVW + 7] < row[payload.C_INVW + 1:payload.C_INVW + 7]).all()


def test_4096_rows_take_seconds_not_minutes():
    from nightmare_rl_amd.model import payload
    rng = np.random.default_rng(0)
    t = time.time()
    rows = payload.payload_rows(rng.uniform(0, 1, 4096), rng.uniform(-0.05, 0.05, (4096, 3)))
    dt = time.time() - t
    print(f"4096 rows: {dt:.2f} s")
    assert rows.shape == (4096, 20) and np.isfinite(rows).all() and dt < 20.0          # 4096 calls of the per-env path: about 100 s


@pytest.mark.parametrize("dm,r,word", [
    (float("nan"), (0, 0, 0), "finite"), (0.1, (0, float("inf"), 0), "finite"),
    (-1.8, (0, 0, 0), "mass must stay positive"), (-1.7287, (0, 0, 0), "mass must stay positive"),
    (-1.0, (0.2, 0, 0), "positive definite"),
    (-0.15, (0, 0, 0.07), "triangle inequality"),
])
def test_inadmissible_payloads_are_refused(dm, r, word):
    from nightmare_rl_amd.model import payload
    with pytest.raises(ValueError, match=word):
        payload.payload_rows([0.0, dm], [[0, 0, 0], list(r)])


def test_shapes_are_checked():
    from nightmare_rl_amd.model import payload
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        payload.payload_rows([0.0, 0.1], [[0, 0, 0]])


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
    for name in ("nm_set_body_params", "nm_get_body_params", "nm_draw_payload"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d4 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 4)
    assert L.nm_set_body_params.argtypes == [vp] * 3
    assert L.nm_get_body_params.argtypes == [vp] * 3
    assert L.nm_draw_payload.argtypes == [vp, d4, d4, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_body_params\(nm_env\* env, const void\* rows_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_get_body_params\(nm_env\* env, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_draw_payload\(nm_env\* env, const double lo\[4\], const double hi\[4\], void\* out_dev, void\* stream\);", hdr)
    # the semantics, and that there is no upstream line
    assert "recompiled with that mass added to base_link" in hdr and "NOTHING stays stale" in hdr and "There is no reference line" in hdr
    assert "added_mass_range" in hdr and "randomize_base_mass" in hdr


def test_a_null_handle_is_refused_by_name(L):
    for fn in ("nm_set_body_params", "nm_get_body_params"):
        assert getattr(L, fn)(None, None, None) != 0
        assert fn.encode() in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
    lo, hi = (ctypes.c_double * 4)(0, 0, 0, 0), (ctypes.c_double * 4)(1, 0, 0, 0)
    assert L.nm_draw_payload(None, ctypes.byref(lo), ctypes.byref(hi), None, None) != 0
    assert b"nm_draw_payload" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()


@pytest.mark.parametrize("lo,hi,word", [
    ((float("nan"), 0, 0, 0), (1, 0, 0, 0), b"dm must be finite"),
    ((0, 0, 0, 0), (float("inf"), 0, 0, 0), b"dm must be finite"),
    ((0, 0, float("-inf"), 0), (1, 0, 0, 0), b"ry must be finite"),
    ((0.5, 0, 0, 0), (0.1, 0, 0, 0), b"lo > hi for dm"),
    ((0, 0.02, 0, 0), (1, 0.01, 0, 0), b"lo > hi for rx"),
    ((0, 0, 0, 0.02), (1, 0, 0, -0.02), b"lo > hi for rz"),
])
def test_bad_ranges_are_refused_before_the_handle_is_looked_at(L, lo, hi, word):
    a, b = (ctypes.c_double * 4)(*lo), (ctypes.c_double * 4)(*hi)
    assert L.nm_draw_payload(None, ctypes.byref(a), ctypes.byref(b), None, None) != 0
    assert word in L.nm_last_error(), L.nm_last_error()


# ---------------------------------------------------------------------------------------------------------------- the config
def _cfg(**kw):
    return types.SimpleNamespace(domain_rand=types.SimpleNamespace(**kw))


def test_optional_domain_rand_is_parsed_into_ranges():
    from nightmare_rl_amd.envs.nightmare_v3_env import payload_config as f
    assert f(types.SimpleNamespace()) == (None, None)
    assert f(_cfg(randomize_base_mass=False, added_mass_range=[-1.0, 1.0])) == (None, None)
    assert f(_cfg(randomize_base_mass=True, added_mass_range=[-0.3, 1.0])) == ((-0.3, 1.0), None)
    assert f(_cfg(randomize_com_displacement=True, com_displacement_range=(-0.03, 0.03))) == (None, (-0.03, 0.03))
    assert f(_cfg(randomize_base_mass=True, added_mass_range=(0.5, 0.5), randomize_com_displacement=True, com_displacement_range=(0, 0.01))) == ((0.5, 0.5), (0.0, 0.01))
    with pytest.raises(ValueError, match="added_mass_range"):
        f(_cfg(randomize_base_mass=True))
    with pytest.raises(ValueError, match="com_displacement_range"):
        f(_cfg(randomize_com_displacement=True))
    for bad in ([1.0, 0.5], [float("nan"), 1.0], [0.0, float("inf")], 3.0, [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="added_mass_range"):
            f(_cfg(randomize_base_mass=True, added_mass_range=bad))
        with pytest.raises(ValueError, match="com_displacement_range"):
            f(_cfg(randomize_com_displacement=True, com_displacement_range=bad))


def test_a_user_subclass_adds_the_ranges_and_the_shipped_config_does_not_have_them():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import env_param_config, payload_config, push_config

    class RandomisedConfig(NightmareV3Config):
        class domain_rand:
            randomize_base_mass, added_mass_range = True, [-0.3, 1.0]
            randomize_com_displacement, com_displacement_range = True, [-0.03, 0.03]

    assert payload_config(RandomisedConfig()) == ((-0.3, 1.0), (-0.03, 0.03))
    assert push_config(RandomisedConfig(), 0.016) == (0, 0.0) and env_param_config(RandomisedConfig()) == (None, None, None)
    assert not hasattr(NightmareV3Config, "domain_rand") and payload_config(NightmareV3Config()) == (None, None)


def test_command_line_flags_exist():
    for path in ("train.py", os.path.join("scripts", "play.py")):
        src = open(os.path.join(ROOT, path)).read()
        assert '"--added-mass-range"' in src and '"--com-range"' in src, path


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
