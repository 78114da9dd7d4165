"""Per-env rows re-drawn at every reset, from pools (nm_set_reset_rows / nm_get_reset_rows / nm_set_reset_row_counts /
nm_get_reset_row_counts / nm_reset_rows_pick, cfg.domain_rand.resample_on_reset): what needs no device - the exports and their ctypes
binding, the refusals that come before any device call, the host's pick against a numpy restatement over oracle.rand_u24 (bits = u 2^24,
exact), the config parser, the pools a config gives, the row helpers the setters and the pools share, and the header's host functions as
a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x524553414D50              # nm::kResetRowsKey, "RESAMP" (nm_reset_rows.h)
KINDS = ("env_params", "base_payload", "action_latency", "gravity", "servo", "torque_limit")
WIDTH = (4, 20, 1, 8, 4, 4)
M64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def restated_pick(seed, genv, k, sizes):
    """i of the six kinds for reset k of the env with global id genv: (bits P) >> 24 in integers, bits = rand_u24(seed + key, genv,
    8 k + kind mod 2^32) 2^24 - 24 bits, exact; a size of 0 gives 0."""
    from oracle import oracle as orc
    out = []
    for kind, P in enumerate(sizes):
        u = orc.rand_u24((seed + KEY) & M64, genv, (8 * k + kind) & 0xFFFFFFFF)
        bits = int(u * 2 ** 24)
        assert bits == u * 2 ** 24 and 0 <= bits < 2 ** 24
        out.append((bits * int(P)) >> 24 if P else 0)
    return out


def library_pick(L, seed, genv, k, sizes):
    s, o = (ctypes.c_uint32 * 6)(*sizes), (ctypes.c_uint32 * 6)()
    assert L.nm_reset_rows_pick(seed, genv, k, ctypes.byref(s), ctypes.byref(o)) == 0, L.nm_last_error()
    return list(o)


def test_library_exports_the_entry_points_with_the_headers_arguments(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ("nm_set_reset_rows", "nm_get_reset_rows", "nm_set_reset_row_counts", "nm_get_reset_row_counts", "nm_reset_rows_pick")
    for name in names:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    vp, i32, u6 = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32 * 6)
    assert L.nm_set_reset_rows.argtypes == [vp, i32, vp, i32, vp]
    assert L.nm_get_reset_rows.argtypes == [vp, i32, ctypes.POINTER(i32), vp, vp]
    assert L.nm_set_reset_row_counts.argtypes == [vp, vp] and L.nm_get_reset_row_counts.argtypes == [vp, vp]
    assert L.nm_reset_rows_pick.argtypes == [ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, u6, u6]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    assert re.search(r"int nm_set_reset_rows\(nm_env\* env, int32_t kind, const void\* rows_dev, int32_t P, void\* stream\);", hdr)
    assert re.search(r"int nm_get_reset_rows\(nm_env\* env, int32_t kind, int32_t\* P, void\* out_dev, void\* stream\);", hdr)
    assert re.search(r"int nm_set_reset_row_counts\(nm_env\* env, const uint32_t\* counts_host\);", hdr)
    assert re.search(r"int nm_get_reset_row_counts\(nm_env\* env, uint32_t\* counts_host\);", hdr)
    assert re.search(r"int nm_reset_rows_pick\(uint64_t seed, int64_t global_env, uint32_t k, const uint32_t sizes\[6\], uint32_t out\[6\]\);", hdr)
    assert "replaces\n * nothing upstream" in hdr and "RESAMP" in hdr and "8 k + kind" in hdr


def test_refusals_come_by_name_before_any_device_call(L):
    rows = (ctypes.c_float * 4)(0.8, 25.0, 0.8, 0.0)         # never read: every call below is refused before the pool is looked at
    p = ctypes.cast(rows, ctypes.c_void_p)
    for kind in (-1, 6, 100):
        assert L.nm_set_reset_rows(None, kind, p, 1, None) != 0
        assert b"nm_set_reset_rows" in L.nm_last_error() and b"kind" in L.nm_last_error()
        assert L.nm_get_reset_rows(None, kind, None, None, None) != 0
        assert b"nm_get_reset_rows" in L.nm_last_error() and b"kind" in L.nm_last_error()
    for P in (0, -3, 65537, 2 ** 31 - 1):
        for kind in range(6):
            assert L.nm_set_reset_rows(None, kind, p, P, None) != 0
            assert b"nm_set_reset_rows" in L.nm_last_error() and b"1..65536" in L.nm_last_error()
    # a null handle is named after the pool's shape has passed; dropping a pool (NULL rows: P is not looked at) needs an env as well
    for kind in range(6):
        for P in (1, 65536):
            assert L.nm_set_reset_rows(None, kind, p, P, None) != 0
            assert b"nm_set_reset_rows" in L.nm_last_error() and b"env is NULL" in L.nm_last_error()
        assert L.nm_set_reset_rows(None, kind, None, 0, None) != 0 and b"env is NULL" in L.nm_last_error()
    n = ctypes.c_int32(7)
    assert L.nm_get_reset_rows(None, 0, ctypes.byref(n), None, None) != 0 and n.value == 7 and b"nm_get_reset_rows" in L.nm_last_error()
    k = (ctypes.c_uint32 * 4)()
    assert L.nm_set_reset_row_counts(None, ctypes.cast(k, ctypes.c_void_p)) != 0 and b"nm_set_reset_row_counts" in L.nm_last_error()
    assert L.nm_get_reset_row_counts(None, ctypes.cast(k, ctypes.c_void_p)) != 0 and b"nm_get_reset_row_counts" in L.nm_last_error()
    s, o = (ctypes.c_uint32 * 6)(1, 1, 1, 1, 1, 65537), (ctypes.c_uint32 * 6)()
    assert L.nm_reset_rows_pick(1, 0, 0, ctypes.byref(s), ctypes.byref(o)) != 0 and b"65536" in L.nm_last_error()
    assert L.nm_reset_rows_pick(1, 0, 0, None, ctypes.byref(o)) != 0 and b"NULL" in L.nm_last_error()


@pytest.mark.parametrize("size", [1, 5, 65536])
def test_host_pick_equals_the_numpy_restatement(L, size):
    seed, sizes = 11, [size] * 6
    seen = {}
    for genv in (0, 62, 4097):
        for k in (0, 1, 2 ** 29):
            got = library_pick(L, seed, genv, k, sizes)
            assert got == restated_pick(seed, genv, k, sizes), (genv, k)
            assert all(0 <= i < size for i in got)
            seen[genv, k] = got
        assert seen[genv, 0] == seen[genv, 2 ** 29]                       # 8 k wraps in 32 bits
    if size == 65536:
        assert seen[0, 0] != seen[0, 1] and seen[0, 0] != seen[62, 0] and len(set(seen[0, 0])) == 6      # every kind its own counter
    mixed = [5, 0, 4, 2, 0, 7]                                            # a kind without a pool reports 0
    for k in (0, 1, 2):
        got = library_pick(L, seed, 9, k, mixed)
        assert got == restated_pick(seed, 9, k, mixed) and got[1] == 0 and got[4] == 0


def _cfg(**kw):
    dr = types.SimpleNamespace(**kw) if kw else None
    return types.SimpleNamespace(**({"domain_rand": dr} if dr is not None else {}))


def test_resample_config_and_each_value_error():
    from nightmare_rl_amd.envs.nightmare_v3_env import RESET_POOL_KINDS, RESET_POOL_WIDTH, resample_config
    assert RESET_POOL_KINDS == KINDS and RESET_POOL_WIDTH == WIDTH and sum(WIDTH) == 41
    assert resample_config(_cfg()) is None and resample_config(_cfg(push_robots=True)) is None
    assert resample_config(_cfg(resample_on_reset=False, resample_pool_size=0)) is None        # off: the size is not looked at
    assert resample_config(_cfg(resample_on_reset=True)) == 1024
    assert resample_config(_cfg(resample_on_reset=True, resample_pool_size=1)) == 1
    assert resample_config(_cfg(resample_on_reset=True, resample_pool_size=np.int64(65536))) == 65536
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="resample_on_reset"):
            resample_config(_cfg(resample_on_reset=bad))
    for bad in (0, -1, 65537, 12.0, "12", True, None):
        with pytest.raises(ValueError, match="resample_pool_size"):
            resample_config(_cfg(resample_on_reset=True, resample_pool_size=bad))


ALL_ON = dict(randomize_friction=True, friction_range=(0.6, 1.2), randomize_gains=True, stiffness_multiplier_range=(0.9, 1.1),
              randomize_base_mass=True, added_mass_range=(-0.1, 0.3), randomize_com_displacement=True, com_displacement_range=(-0.02, 0.02),
              randomize_action_latency=True, action_latency_range=(0, 6), randomize_slope=True, slope_range=(0.0, 0.1),
              randomize_action_rate_limit=True, action_rate_limit_range=(0.2, 0.5), randomize_torque_limit=True,
              torque_limit_range=[[3.0, 6.0], [3.0, 5.0], [3.0, 4.0]])


def test_the_pools_of_a_config_do_not_depend_on_the_rank_and_follow_the_switches():
    """config_pools takes the seed and no env id: two ranks (env_id_offset 0 and 4096) call it with the same arguments, so the test pins
    that it is a pure function of (cfg, seed, size) - and that another seed, and another kind, draw other values."""
    from nightmare_rl_amd.envs import nightmare_v3_env as ev
    import inspect
    assert list(inspect.signature(ev.config_pools).parameters) == ["cfg", "seed", "size", "envp_default"]
    src = inspect.getsource(ev.NightmareV3Env.__init__)
    assert "config_pools(cfg, seed, resample_size, self._envp_default)" in src                 # env_id_offset does not enter
    dflt = (1.0, 25.0, 0.8)
    a = ev.config_pools(_cfg(resample_on_reset=True, **ALL_ON), 7, 16, dflt)
    b = ev.config_pools(_cfg(resample_on_reset=True, **ALL_ON), 7, 16, dflt)
    c = ev.config_pools(_cfg(resample_on_reset=True, **ALL_ON), 8, 16, dflt)
    assert list(a) == list(KINDS)
    for kind in KINDS:
        for name in a[kind]:
            x, y, z = a[kind][name], b[kind][name], c[kind][name]
            if x is None:
                assert y is None
                continue
            np.testing.assert_array_equal(x, y)
            assert len(x) in (16, 3) and (len(x) == 3 or not np.array_equal(x, z)), (kind, name)
    e = a["env_params"]
    assert e["mu"].dtype == np.float64 and e["mu"].min() >= 0.6 and e["mu"].max() < 1.2 and e["kv"] is None
    assert e["p_gain"].min() >= 0.9 * 25 and e["p_gain"].max() < 1.1 * 25
    assert a["action_latency"]["substeps"].dtype == np.int32 and set(a["action_latency"]["substeps"]) <= set(range(7))
    g = a["gravity"]["g"]
    np.testing.assert_allclose(np.linalg.norm(g, axis=1), 9.81, rtol=1e-12)
    assert a["gravity"]["gravity_vec"] is None and (np.arccos(-g[:, 2] / 9.81) <= 0.1 + 1e-12).all()
    t = a["torque_limit"]["limit"]
    assert t.shape == (16, 3) and (t >= 3.0).all() and (t[:, 2] < 4.0).all()
    assert not np.array_equal(a["env_params"]["mu"][:3], a["servo"]["rate_limit"][:3])        # every kind its own generator
    # only the switches that are on get a pool; fixed cfg.control values are not randomisation
    some = ev.config_pools(_cfg(resample_on_reset=True, randomize_friction=True, friction_range=(0.5, 0.9)), 7, 4, dflt)
    assert list(some) == ["env_params"] and some["env_params"]["p_gain"] is None
    cfg = _cfg(resample_on_reset=True)
    cfg.control = types.SimpleNamespace(action_rate_limit=0.3, torque_limit=3.2)
    assert ev.config_pools(cfg, 7, 4, dflt) == {}


def test_the_row_helpers_give_the_rows_the_setters_send():
    """The helpers the setters and set_reset_pool share, on the CPU, against the arrays the setters formed before they were factored out."""
    import torch
    from nightmare_rl_amd.envs import nightmare_v3_env as ev
    from nightmare_rl_amd.model import payload
    n, rng = 5, np.random.default_rng(3)
    for real in (torch.float32, torch.float64):
        mu, kv = rng.uniform(0.5, 1.0, n), 0.7
        cols = ev.env_param_columns(n, real, "cpu", mu, None, kv, "e")
        assert cols[1] is None and cols[0].dtype == real and torch.equal(cols[0], torch.as_tensor(mu, dtype=real))
        assert torch.equal(cols[2], torch.full((n,), 0.7, dtype=real))
        rows = ev.env_param_rows(cols, (1.0, 25.0, 0.8), n, real, "cpu")
        want = torch.zeros(n, 4, dtype=real)
        want[:, 0], want[:, 1], want[:, 2] = torch.as_tensor(mu, dtype=real), 25.0, 0.7
        assert torch.equal(rows, want)
        with pytest.raises(ValueError, match="^e$"):
            ev.env_param_columns(n, real, "cpu", [1.0, 2.0], None, None, "e")
        # servo: None = (inf, 0)
        rate = rng.uniform(0.2, 0.5, n)
        s = ev.servo_rows(n, real, "cpu", rate, None, "e")
        want = torch.zeros(n, 4, dtype=real)
        want[:, 0] = torch.as_tensor(rate, dtype=real)
        assert torch.equal(s, want)
        s = ev.servo_rows(n, real, "cpu", None, 0.25, "e")
        assert torch.isinf(s[:, 0]).all() and (s[:, 1] == 0.25).all() and not s[:, 2:].any()
        # torque: a scalar, 3 values, [n], [n, 3]
        for lim, want3 in ((3.0, np.full((n, 3), 3.0)), ([6.0, 4.0, 3.0], np.tile([6.0, 4.0, 3.0], (n, 1))),
                           (np.arange(1.0, n + 1), np.tile(np.arange(1.0, n + 1)[:, None], (1, 3))), (np.arange(1.0, 3 * n + 1).reshape(n, 3),) * 2):
            t = ev.torque_rows(n, real, "cpu", lim, "e")
            assert t.dtype == real and torch.equal(t[:, :3], torch.as_tensor(want3, dtype=real)) and not t[:, 3].any()
        with pytest.raises(ValueError, match="^e$"):
            ev.torque_rows(n, real, "cpu", np.ones((n, 2)), "e")
    # payload: (dm, r) -> model/payload.py's rows; a scalar dm and one r for all
    dm, r = rng.uniform(-0.1, 0.3, n), rng.uniform(-0.02, 0.02, (n, 3))
    d2, r2 = ev.payload_values(n, dm, r, "e")
    np.testing.assert_array_equal(d2, dm)
    np.testing.assert_array_equal(r2, r)
    np.testing.assert_array_equal(ev.payload_body_rows(d2, r2), payload.payload_rows(dm, r))
    d3, r3 = ev.payload_values(n, 0.2, [0.01, 0.0, -0.01], "e")
    np.testing.assert_array_equal(d3, np.full(n, 0.2))
    np.testing.assert_array_equal(r3, np.tile([0.01, 0.0, -0.01], (n, 1)))
    assert ev.payload_values(n, 0.2, None, "e")[1].shape == (n, 3)
    with pytest.raises(ValueError, match="^e$"):
        ev.payload_values(n, dm, np.zeros((n + 1, 3)), "e")
    # gravity: g[3] pad gravity_vec[3] pad; None = g
    g = ev.gravity_from_draw(np.zeros((n, 3)), rng.uniform(0, 0.1, n), rng.uniform(0, 6.28, n))
    rows = ev.gravity_rows(n, g, None, "e")
    assert rows.shape == (n, 8) and np.array_equal(rows[:, 0:3], g) and np.array_equal(rows[:, 4:7], g) and not rows[:, [3, 7]].any()
    rows = ev.gravity_rows(n, g, [0.0, 0.0, -9.81], "e")
    assert np.array_equal(rows[:, 4:7], np.tile([0.0, 0.0, -9.81], (n, 1)))
    with pytest.raises(ValueError, match="^e$"):
        ev.gravity_rows(n, g[:-1], None, "e")
    # latency: integers only
    d = ev.latency_values(n, "cpu", [0, 1, 2, 3, 6], "who")
    assert d.dtype == torch.int32 and d.tolist() == [0, 1, 2, 3, 6]
    assert ev.latency_values(n, "cpu", 4, "who").tolist() == [4] * n
    with pytest.raises(ValueError, match="who: whole substeps"):
        ev.latency_values(n, "cpu", [0.5] * n, "who")
    with pytest.raises(ValueError, match="who: one delay per env"):
        ev.latency_values(n, "cpu", [1, 2], "who")


def test_the_shipped_config_tree_and_the_command_line():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import resample_config
    assert not hasattr(NightmareV3Config, "domain_rand") and resample_config(NightmareV3Config()) is None
    for f in ("train.py", os.path.join("scripts", "play.py")):
        assert "--resample-on-reset" in open(os.path.join(ROOT, f)).read(), f


def test_the_headers_host_functions_as_a_stand_alone_program_under_the_sanitizers(L, tmp_path):
    """tests/tools/reset_rows_host_main.cpp (its own main, -DNM_EMUL: no device code) under -fsanitize=address,undefined: the lane map,
    nm_reset_rows_pick for k = 0, 1, 2^29 and sizes 1, 5, 65536 and a mixed set against the restatement, and the admission of a pool
    row by every kind's own rule - one admissible pool and the rows each rule rejects, in both dtypes."""
    exe = str(tmp_path / "reset_rows_host")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces", "-DNM_EMUL", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "tools", "reset_rows_host_main.cpp")])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    lines = out.stdout.splitlines()
    assert lines[0] == "first 0 4 24 25 33 37 41"
    assert lines[1] == "map " + " ".join(str(k) for k, w in enumerate(WIDTH) for _ in range(w))
    picks = [ln for ln in lines if ln.startswith("pick")]
    assert len(picks) == 36
    for ln in picks:
        a, b = ln[5:].split(" : ")
        seed, genv, k, *sizes = (int(x) for x in a.split())
        assert [int(x) for x in b.split()] == restated_pick(seed, genv, k, sizes) == library_pick(L, seed, genv, k, sizes), ln
    faults = {tuple(ln[6:].split(" : ")[0].split()): ln.split(" : ")[1] for ln in lines if ln.startswith("fault")}
    words = {("0", "mu"): "mu must be above 1e-5", ("0", "p_gain"): "p_gain must not be negative", ("0", "kv"): "kv must not be negative",
             ("0", "nan"): "non-finite", ("1", "mass"): "mass <= 0", ("1", "total"): "total_mass < mass", ("1", "nan"): "non-finite",
             ("1", "pgs"): "pgs_scale", ("3", "zero_vec"): "zero gravity_vec", ("3", "nan"): "non-finite", ("4", "rate"): "rate not > 0",
             ("4", "d_gain"): "d_gain", ("4", "nan"): "rate not > 0", ("5", "limit"): "limit 1 not > 0", ("5", "nan"): "limit 2 not > 0"}
    for dt in ("f32", "f64"):
        for kind in "01345":
            assert faults[kind, dt, "good"] == "ok"
        for (kind, case), word in words.items():
            assert faults[kind, dt, case].startswith("row 2: ") and word in faults[kind, dt, case], (kind, dt, case)
    assert faults["2", "i32", "good"] == "ok"
    assert "delay 7 outside [0, 6]" in faults["2", "i32", "above"] and "delay -1 outside" in faults["2", "i32", "below"]
    assert len(faults) == 2 * (5 + len(words)) + 3
