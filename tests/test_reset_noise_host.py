"""Randomised reset states (nm_set_reset_noise / nm_get_reset_noise / nm_reset_noise_offsets, the optional cfg.domain_rand): what needs no
device - the exports and their ctypes binding, the refusals that come before any device call, the config parser, the host's draw against
a numpy restatement over oracle.rand_u24 BIT FOR BIT, and the config classes' dump, which the feature must not touch."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESET_KEY = 0x5245534554         # nm::kResetKey (nm_reset_noise.h)
NCOL = 43
RANGES = np.array([[-0.02, 0.03], [-0.25, 0.2], [-0.5, 0.4], [-0.3, 0.6], [-1.0, 1.5]])


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def col_range(c):
    """the range of column c: base_height | 18 x dof_pos | 3 x base_lin_vel | 3 x base_ang_vel | 18 x dof_vel"""
    return 0 if c == 0 else 1 if c < 19 else 2 if c < 22 else 3 if c < 25 else 4


def restated_offsets(ranges, seed, genv, k, dtype):
    """d(0..42) of reset k of the env with global id genv: lo_r + u * w_r in `dtype`, product and sum rounded separately (numpy scalars
    round every operation), u = rand_u24(seed + kResetKey, genv, 64 k + c mod 2^32) - 24 bits, exact in both dtypes."""
    from oracle import oracle as orc
    r = np.asarray(ranges, np.float64).reshape(5, 2)
    out = np.zeros(NCOL, dtype)
    for c in range(NCOL):
        lo, hi = dtype(r[col_range(c), 0]), dtype(r[col_range(c), 1])
        w = dtype(hi - lo)
        u = dtype(orc.rand_u24((seed + RESET_KEY) & (2 ** 64 - 1), genv, (64 * k + c) & 0xFFFFFFFF))
        out[c] = dtype(lo + dtype(u * w))
    return out


def library_offsets(L, ranges, seed, genv, k, dtype_code):
    r = (ctypes.c_double * 10)(*np.asarray(ranges, np.float64).reshape(-1))
    out = (ctypes.c_double * NCOL)()
    rc = L.nm_reset_noise_offsets(ctypes.byref(r), seed, genv, k, dtype_code, ctypes.byref(out))
    assert rc == 0, L.nm_last_error()
    return np.array(out[:], np.float64)


def test_library_exports_the_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_set_reset_noise", "nm_get_reset_noise", "nm_reset_noise_offsets"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, d10 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double * 10)
    assert L.nm_set_reset_noise.argtypes == [vp, d10, vp]
    assert L.nm_get_reset_noise.argtypes == [vp, ctypes.POINTER(ctypes.c_int32), d10, vp]
    assert L.nm_reset_noise_offsets.argtypes == [d10, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(ctypes.c_double * NCOL)]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_reset_noise\(nm_env\* env, const double\* ranges10_host, const uint32_t\* counts_host\);", hdr)
    assert re.search(r"int nm_get_reset_noise\(nm_env\* env, int32_t\* on, double\* ranges10, uint32_t\* counts_host\);", hdr)
    assert re.search(r"int nm_reset_noise_offsets\(const double\* ranges10, uint64_t seed, int64_t global_env, uint32_t k, int32_t dtype, double\* out43\);", hdr)
    assert "the reference has no such line" in hdr and "_reset_dofs" in hdr and "_reset_root_states" in hdr


def test_refusals_come_by_name_before_any_device_call(L):
    good = (ctypes.c_double * 10)(*RANGES.reshape(-1))
    assert L.nm_set_reset_noise(None, ctypes.byref(good), None) != 0
    assert b"nm_set_reset_noise" in L.nm_last_error() and b"env" in L.nm_last_error()
    assert L.nm_set_reset_noise(None, None, None) != 0                       # switching off needs an env as well
    assert b"nm_set_reset_noise" in L.nm_last_error() and b"env" in L.nm_last_error()
    on = ctypes.c_int32(7)
    assert L.nm_get_reset_noise(None, ctypes.byref(on), None, None) != 0 and on.value == 7
    assert b"nm_get_reset_noise" in L.nm_last_error() and b"env" in L.nm_last_error()
    names = ("base_height", "dof_pos", "base_lin_vel", "base_ang_vel", "dof_vel")
    out = (ctypes.c_double * NCOL)()
    for k, name in enumerate(names):
        for bad, word in ((float("nan"), b"finite"), (float("inf"), b"finite"), (None, b"lo > hi")):
            r = RANGES.copy()
            if bad is None:
                r[k] = (0.2, 0.1)
            else:
                r[k, 1] = bad
            arr = (ctypes.c_double * 10)(*r.reshape(-1))
            # the ranges are judged before the handle, so a bad range is named whatever the handle is
            assert L.nm_set_reset_noise(None, ctypes.byref(arr), None) != 0
            err = L.nm_last_error()
            assert b"nm_set_reset_noise" in err and word in err and name.encode() in err, err
            for code in (0, 1):
                assert L.nm_reset_noise_offsets(ctypes.byref(arr), 1, 0, 0, code, ctypes.byref(out)) != 0
                err = L.nm_last_error()
                assert b"nm_reset_noise_offsets" in err and word in err and name.encode() in err, err
    assert L.nm_reset_noise_offsets(ctypes.byref(good), 1, 0, 0, 2, ctypes.byref(out)) != 0 and b"dtype" in L.nm_last_error()
    assert L.nm_reset_noise_offsets(None, 1, 0, 0, 0, ctypes.byref(out)) != 0 and b"NULL" in L.nm_last_error()
    big = RANGES.copy()
    big[4] = (-1e39, 1e39)                                                    # finite in double, not in float32
    arr = (ctypes.c_double * 10)(*big.reshape(-1))
    assert L.nm_reset_noise_offsets(ctypes.byref(arr), 1, 0, 0, 1, ctypes.byref(out)) == 0
    assert L.nm_reset_noise_offsets(ctypes.byref(arr), 1, 0, 0, 0, ctypes.byref(out)) != 0 and b"dof_vel" in L.nm_last_error()


def _cfg(**kw):
    dr = types.SimpleNamespace(**kw) if kw else None
    return types.SimpleNamespace(**({"domain_rand": dr} if dr is not None else {}))


def test_optional_domain_rand_is_parsed_into_five_ranges():
    from nightmare_rl_amd.envs.nightmare_v3_env import RESET_NOISE_RANGES, reset_noise_config
    assert RESET_NOISE_RANGES == ("reset_base_height_range", "reset_dof_pos_range", "reset_base_lin_vel_range", "reset_base_ang_vel_range",
                                  "reset_dof_vel_range")
    assert reset_noise_config(_cfg()) is None                                                          # no class at all
    assert reset_noise_config(_cfg(push_robots=True)) is None                                          # a class without the flag
    assert reset_noise_config(_cfg(randomize_reset_state=False, reset_dof_pos_range=(-0.1, 0.1))) is None
    assert reset_noise_config(_cfg(randomize_reset_state=True, reset_dof_pos_range=(-0.1, 0.2))) == \
        ((0.0, 0.0), (-0.1, 0.2), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))                                  # a missing range is (0, 0)
    full = dict(zip(RESET_NOISE_RANGES, ([-0.01, 0.02], (-0.1, 0.2), (-0.3, 0.3), (-0.4, 0.5), (0, 1))))
    assert reset_noise_config(_cfg(randomize_reset_state=True, **full)) == ((-0.01, 0.02), (-0.1, 0.2), (-0.3, 0.3), (-0.4, 0.5), (0.0, 1.0))
    with pytest.raises(ValueError, match="randomize_reset_state needs"):
        reset_noise_config(_cfg(randomize_reset_state=True))                                           # the flag without a range
    for bad in ((0.2, 0.1), (0.0, float("nan")), (0.0, float("inf")), 0.3, (0.1, 0.2, 0.3), "ab"):
        with pytest.raises(ValueError, match="reset_dof_vel_range"):
            reset_noise_config(_cfg(randomize_reset_state=True, reset_dof_vel_range=bad))


@pytest.mark.parametrize("code,dtype", [(0, np.float32), (1, np.float64)])
def test_host_draw_equals_the_numpy_restatement_bit_for_bit(L, code, dtype):
    seed = 11
    seen = {}
    for genv in (0, 4097):
        for k in (0, 1, 2 ** 26):
            got = library_offsets(L, RANGES, seed, genv, k, code)
            want = restated_offsets(RANGES, seed, genv, k, dtype)
            np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"env {genv} reset {k}")
            assert got.astype(dtype).astype(np.float64).tobytes() == got.tobytes()                     # values of the env's precision
            for c in range(NCOL):
                lo, hi = RANGES[col_range(c)]
                assert dtype(lo) <= got[c] <= dtype(hi)
            seen[genv, k] = got
    for genv in (0, 4097):
        np.testing.assert_array_equal(seen[genv, 0], seen[genv, 2 ** 26])                              # 64 k wraps in 32 bits
        assert (seen[genv, 0] != seen[genv, 1]).all()
    assert (seen[0, 0] != seen[4097, 0]).all()
    assert len(set(seen[0, 0][1:19])) == 18                                                            # every column its own counter


@pytest.mark.parametrize("code", [0, 1])
def test_zero_ranges_give_43_positive_zeros(L, code):
    got = library_offsets(L, np.zeros((5, 2)), 11, 5, 3, code)
    assert got.tobytes() == np.zeros(NCOL).tobytes()                                                   # +0, not -0
    one = np.zeros((5, 2))
    one[1] = (-0.1, 0.1)
    got = library_offsets(L, one, 11, 5, 3, code)
    assert (got[1:19] != 0).all() and got[0] == 0 and (got[19:] == 0).all()


def test_config_classes_still_dump_exactly_the_golden_tree():
    """class_to_dict of the shipped config classes against tests/golden/config_class_to_dict.json, as test_abi_and_host.py compares them
    (that test remains the yardstick): the feature adds no attribute to the pinned tree."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
    from nightmare_rl_amd.envs.nightmare_v3_env import reset_noise_config
    assert not hasattr(NightmareV3Config, "domain_rand") and reset_noise_config(NightmareV3Config()) is None
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "config_class_to_dict.json")))
    ours = {"NightmareV3Config": class_to_dict(NightmareV3Config()), "NightmareV3ConfigPPO": class_to_dict(NightmareV3ConfigPPO())}
    assert "domain_rand" not in ours["NightmareV3Config"] and "domain_rand" not in ref["NightmareV3Config"]
    # the three defaults this backend changes on purpose
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
