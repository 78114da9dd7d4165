"""Per-env gravity vectors (nm_set_gravity / nm_get_gravity / nm_draw_gravity) on the device, in every stepping path.
References: the fp64 fixture of the oracle's gravity rows (tests/golden/gravity.npz, make_gravity_goldens.py: the physics gravity per env;
for the observed sets the env layer's gravity_vec as well, for the other one upstream's constant) for what the rows mean;
uniform batches for what a mixed batch must give (bit for bit: every env is independent); the per-step path for the K-step launches (bit
for bit); a numpy restatement over oracle.rand_u24 for the draw; closed-form free flight and a numpy rotation for two known answers that
do not go through the oracle. The file mirrors tests/test_gpu_payload.py group for group."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_env_params import DBG_NCON, DBG_NTOG, forced, free, load_state, set_of
from test_gpu_parity import make_env
from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_push import _actions, _assert_same_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step
from test_gravity_host import draw_restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
POPS = ("drop", "stand", "belly")
H = 0.008      # the model's timestep
ENVP_SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])


@pytest.fixture(scope="module")
def G():
    return load_golden("gravity.npz")


def set_gravity(env, g, sets):
    r = g["rows"][np.asarray(sets)]
    env.set_gravity(r[:, 0:3], r[:, 4:7])


def set_every_other_kind(env, N, push=True):
    sets = set_of(N)
    r = ENVP_SETS[(sets + 1) % 4]
    env.set_env_params(mu=r[:, 0], p_gain=r[:, 1], kv=r[:, 2])
    env.set_base_payload(np.array([0.0, 0.5, -0.3, 1.0])[(sets + 2) % 4], np.array([[0, 0, 0], [0.03, 0, 0.04], [0, 0, 0], [-0.05, 0.02, 0.05]], float)[(sets + 2) % 4])
    env.set_action_latency(torch.arange(N, dtype=torch.int32) % 7)
    if push:
        env.set_push(3, 0.5)


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the variant oracles
def test_fp64_kernel_with_mixed_gravity_matches_the_variant_oracles(G):
    """N = 32, the four sets mixed over the envs. Teacher-forced single steps and the free-running trajectories of all three
    populations: obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py), no done flag differing."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_gravity(env, G, sets)
    T = G["drop_actions"].shape[1]
    for pop in POPS:
        err, serr, flags = forced(env, G, pop, sets, T)
        print(f"{pop} forced: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, err.max(), serr)
        err, serr, flags = free(env, G, pop, sets, T)
        print(f"{pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, "free", err.max(), serr)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. mixed batch = uniform batches
def _run8(env, g, pop, sets, dbg=None):
    """8 free-running steps from the fixture's start states; every step's (obs, rew, done) and state."""
    out = []
    load_state(env, g, pop, 0, sets)
    ev = np.arange(len(sets)) % 8
    ntog = nbig = 0
    for t in range(8):
        env.set_command_uniforms(g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64))
        r = env.step(torch.from_numpy(g[f"{pop}_actions"][sets, t, ev]))
        out.append((r[0].cpu().numpy().copy(), r[2].cpu().numpy().copy(), r[3].cpu().numpy().copy()) + tuple(env.get_state()))
        if dbg is not None:
            d = dbg.cpu().numpy()
            ntog += int(d[0::2, DBG_NTOG].sum())
            nbig += int((d[:, DBG_NCON] > 16).sum())      # ncon > kMaxCon (16) IS the dispatch to stage_constraint_big (nm_core.h stage_constraint)
    return out, ntog, nbig


@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (63, torch.float64), (1, torch.float32), (1, torch.float64)])
def test_mixed_batch_equals_uniform_batches_bit_for_bit(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL carry e's gravity rows (same states, same actions): what differs
    between the runs is only what e's wave neighbour carries. 8 steps per population. N = 63: 31 full waves and a half-filled one; the
    fp32 kernel must have taken both envs of a wave through ONE constraint pass, and both kernels an env-step above 16 contacts."""
    sets = set_of(N) if N > 1 else np.array([3])
    mixed = make_env(N, dtype=dtype, seed=SEED)
    set_gravity(mixed, G, sets)
    dbg = torch.zeros((N, 256), dtype=dtype, device=DEV)
    mixed.set_debug_buffer(dbg)
    runs, ntog, nbig = {}, 0, 0
    for pop in POPS:
        runs[pop], a, b = _run8(mixed, G, pop, sets, dbg)
        ntog += a; nbig += b
    mixed.set_debug_buffer(None)
    mixed.close()
    print(f"N {N} {dtype}: two-env constraint passes {ntog}, env-steps above 16 contacts {nbig}")
    if N > 1:
        assert nbig >= 1
        if dtype == torch.float32:
            assert ntog >= 1
    for k in sorted(set(sets.tolist())):
        uni = make_env(N, dtype=dtype, seed=SEED)
        set_gravity(uni, G, np.full(N, k))
        m = sets == k
        for pop in POPS:
            other, _, _ = _run8(uni, G, pop, sets)
            for t, (x, y) in enumerate(zip(runs[pop], other)):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart"), x, y):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} {pop} step {t} {name}")
        uni.close()


# ------------------------------------------------------------------------------------------------ 3. fp32 kernel vs the fixture
def test_fp32_kernel_with_mixed_gravity_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps, N = 32: median < 5e-6, p99 < 1e-4 (the bounds of tests/test_gpu_env_params.py for the fp32 kernel; the
    fp32 emulation of these very states stays inside them, tests/test_gravity_emulated.py)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float32, seed=SEED)
    set_gravity(env, G, sets)
    errs = []
    for pop in POPS:
        err, _, flags = forced(env, G, pop, sets, G[f"{pop}_actions"].shape[1])
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 4. off = default rows
@pytest.mark.parametrize("others", [False, True], ids=["alone", "with_friction_payload_latency"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_off_equals_default_rows_under_equality(G, dtype, others):
    """Never set, (0, 0, -9.81) twice in every env set explicitly (level 4), and set then cleared: equal under == in every output over
    8 steps of each population; alone, and with friction, payload and latency all on. Rows the library refuses change nothing."""
    from nightmare_rl_amd import _lib
    N = 16
    sets = np.zeros(N, int)
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        if others:
            set_every_other_kind(e, N, push=False)
    off = envs[0].gravity()
    assert off["g"].dtype == dtype and off["g"].shape == (N, 3)
    want = torch.tensor([0.0, 0.0, -9.81], dtype=dtype, device=DEV).expand(N, 3)
    assert torch.equal(off["g"], want) and torch.equal(off["gravity_vec"], want)
    envs[1].set_gravity([0.0, 0.0, -9.81])
    envs[2].set_gravity(G["rows"][1, 0:3])
    assert not torch.equal(envs[2].gravity()["g"], want)
    for bad_g, bad_v, word in (([0.0, float("nan"), -9.81], None, "non-finite"), ([0.0, 0.0, -9.81], [float("inf"), 0.0, 0.0], "non-finite"),
                               ([1.0, 0.0, -9.0], [0.0, 0.0, 0.0], "zero gravity_vec")):
        with pytest.raises(_lib.NightmareHipError, match=word):
            envs[2].set_gravity(bad_g, bad_v)
    np.testing.assert_allclose(envs[2].gravity()["g"][3].cpu().numpy(), G["rows"][1, 0:3], rtol=1e-6)      # a refused call changed nothing
    envs[2].set_gravity([0.0, 0.0, 0.0], [0.0, 0.0, -9.81])      # a zero g is admitted: free float
    envs[2].set_gravity(None)
    for e in envs:
        assert torch.equal(e.gravity()["g"], want) and torch.equal(e.gravity()["gravity_vec"], want)
    for pop in POPS:
        runs = [_run8(e, G, pop, sets)[0] for e in envs]
        for other, what in ((runs[1], "default rows"), (runs[2], "set then cleared")):
            for t, (x, y) in enumerate(zip(runs[0], other)):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart"), x, y):
                    np.testing.assert_array_equal(u, v, err_msg=f"{what} {pop} step {t} {name}")
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. every stepping path
def _mixed(G, N, n, others):
    envs = [make_env(N, seed=SEED) for _ in range(n)]
    for e in envs:
        e.reset()
        set_gravity(e, G, set_of(N))
        if others:
            set_every_other_kind(e, N)
    return envs


@pytest.mark.parametrize("others", [False, True], ids=["alone", "every_other_kind_and_push"])
def test_tape_with_gravity_equals_the_per_step_path(G, others):
    N, K = 16, 10
    ea, eb, e0 = _mixed(G, N, 3, others)
    e0.set_gravity(None)
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec, rec0 = _records(K, N), _records(K, N)
    oa = ea.step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(eb, acts, bb, ep_idx)
    e0.step_tape(acts, record=rec0)
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    m = torch.from_numpy(set_of(N) != 0).to(DEV)
    assert not torch.equal(rec["obs"][-1][m], rec0["obs"][-1][m])               # the rows were honoured
    assert torch.equal(rec["obs"][-1][~m], rec0["obs"][-1][~m])                 # ... and the envs of set 0 carry the nominal vectors: untouched
    for e in (ea, eb, e0):
        e.close()


def _assert_rows_honoured(N, with_rows, cleared):
    """Final observations of the launch with the gravity rows against the same launch with gravity cleared (every other kind as it
    was): the envs of a non-default set differ, the envs of set 0 carry the nominal vectors and do not."""
    m = torch.from_numpy(set_of(N) != 0).to(DEV)
    assert not torch.equal(with_rows[m], cleared[m])
    assert torch.equal(with_rows[~m], cleared[~m])


@pytest.mark.parametrize("others", [False, True], ids=["alone", "every_other_kind_and_push"])
@pytest.mark.parametrize("deterministic", [True, False])
def test_play_with_gravity_equals_the_per_step_path(G, deterministic, others):
    N, K = 16, 10
    ac, fu = _networks()
    ea, eb = _mixed(G, N, 2, others)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    if others:
        e0, = _mixed(G, N, 1, True)
        e0.set_gravity(None)
        o0 = e0.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it)
        torch.cuda.synchronize()
        _assert_rows_honoured(N, oa, o0)
        e0.close()
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("others", [False, True], ids=["alone", "every_other_kind_and_push"])
def test_rollout_with_gravity_equals_the_per_step_path(G, others):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, T, gamma = 16, 10, 0.99
    ac, fu = _networks()
    ea, eb = _mixed(G, N, 2, others)
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    sa, sb = _storage(N, T), _storage(N, T)
    oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]))
    o = eb.get_observations()
    for s in range(T):
        act = eb.policy_act(fu.flat, o, 99, it, s, sb)
        o, _, rew, done, infos = eb.step(act)
        _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
    torch.cuda.synchronize()
    for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(sa, name), getattr(sb, name)), name
    _assert_same_env(ea, eb, oa, o)
    assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
    if others:
        e0, = _mixed(G, N, 1, True)
        e0.set_gravity(None)
        b0, s0 = _books(N, ep_idx.numel()), _storage(N, T)
        o0 = e0.policy_rollout(T, fu.flat, 99, it, s0, gamma, b0["cur_ret"], b0["cur_len"], b0["fin"], ep=(ep_idx, b0["ep_acc"]))
        torch.cuda.synchronize()
        _assert_rows_honoured(N, oa, o0)
        e0.close()
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 6. physics-only ignores latency at level 4
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_step_physics_with_gravity_ignores_latency(G, dtype):
    N = 16
    ea, eb = (make_env(N, dtype=dtype, seed=SEED) for _ in range(2))
    for e in (ea, eb):
        e.reset()
        set_gravity(e, G, set_of(N))
    ea.set_action_latency(torch.arange(N, dtype=torch.int32) % 7)
    hist = ea.action_history().clone()
    acts = _actions(4, N)
    for s in range(4):
        ea.step_physics(acts[s]); eb.step_physics(acts[s])
    for name, x, y in zip(("qpos", "qvel", "qacc_warmstart"), ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert torch.equal(ea.action_history(), hist)
    ra, rb = ea.step(acts[0]), eb.step(acts[0])      # ... and a full step does not: the delayed envs part from the undelayed ones
    assert not torch.equal(ra[0], rb[0])
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 7. the draw
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_draw_is_its_numpy_restatement_and_lies_in_range(dtype):
    from nightmare_rl_amd import _lib
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_from_draw
    N, npdt = 1024, (np.float64 if dtype == torch.float64 else np.float32)
    env = make_env(N, dtype=dtype, seed=SEED, env_id_offset=1000)
    of, ti = (-1.0, 1.0), (0.0, 0.3)
    p = env.draw_gravity(offset_range=of, tilt_range=ti)
    d = draw_restated(SEED, 1000 + np.arange(N), [of[0]] * 3 + [ti[0], 0.0], [of[1]] * 3 + [ti[1], 2.0 * np.pi], npdt).astype(np.float64)
    want = torch.from_numpy(gravity_from_draw(d[:, 0:3], d[:, 3], d[:, 4])).to(dtype)
    assert torch.equal(p["g"].cpu(), want) and torch.equal(p["gravity_vec"].cpu(), want)
    assert d[:, 3].min() >= 0 and d[:, 3].max() <= npdt(0.3) and d[:, 3].max() - d[:, 3].min() > 0.29
    assert d[:, 4].min() >= 0 and d[:, 4].max() < 2 * np.pi + 1e-6 and d[:, 4].max() - d[:, 4].min() > 6.2
    tilt = np.arccos(np.clip(-(p["g"].cpu().numpy().astype(np.float64) - d[:, 0:3])[:, 2] / 9.81, -1.0, 1.0))
    assert np.abs(tilt - d[:, 3]).max() < 1e-3      # (fp32: acos near 1 turns the rounding of g, 2^-24 relative, into sqrt(2 x 2^-23) = 5e-4 rad)
    # no tilt range: no azimuth either, g = (0, 0, -9.81) + offset; not observed: the env layer keeps upstream's constant
    q = env.draw_gravity(offset_range=of, observed=False)
    np.testing.assert_array_equal(q["g"].cpu().numpy()[:, 0], d[:, 0].astype(npdt))
    assert torch.equal(q["gravity_vec"], torch.tensor([0.0, 0.0, -9.81], dtype=dtype, device=DEV).expand(N, 3))
    # refusals before any device call; a refused call changes nothing
    for kw in (dict(offset_range=(0.5, 0.1)), dict(offset_range=(0.0, float("inf")))):
        with pytest.raises(_lib.NightmareHipError, match="nm_draw_gravity"):
            env.draw_gravity(**kw)
    for bad in ((0.2, 0.1), (-0.1, 0.1), (0.0, 1.6)):
        with pytest.raises(ValueError, match="tilt_range"):
            env.draw_gravity(tilt_range=bad)
    assert torch.equal(env.gravity()["g"], q["g"])
    assert env.gravity_vec.tolist() == [0.0, 0.0, -9.81]      # the reference attribute stays the constant array
    env.close()


def test_drawn_gravity_and_results_do_not_depend_on_sharding():
    whole = make_env(128, seed=SEED)
    parts = [make_env(64, seed=SEED, env_id_offset=off) for off in (0, 64)]
    for e in [whole] + parts:
        e.reset()
        e.draw_gravity(offset_range=(-0.5, 0.5), tilt_range=(0.0, 0.25))
    pw, pp = whole.gravity(), [p.gravity() for p in parts]
    assert torch.equal(pw["g"], torch.cat([p["g"] for p in pp]))
    assert pw["g"].unique(dim=0).shape[0] == 128
    acts = _actions(8, 128)
    for s in range(8):
        rw = whole.step(acts[s])
        rp = [p.step(acts[s, 64 * i:64 * (i + 1)].contiguous()) for i, p in enumerate(parts)]
        torch.cuda.synchronize()
        for k in (0, 2, 3):
            assert torch.equal(rw[k], torch.cat([r[k] for r in rp])), (s, k)
        for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
            np.testing.assert_array_equal(x, np.concatenate(ys), err_msg=f"step {s}")
    for e in [whole] + parts:
        e.close()


def test_cfg_domain_rand_draws_at_construction():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

    class Cfg(NightmareV3Config):
        class domain_rand:
            randomize_gravity, gravity_range = True, [-1.0, 1.0]
            randomize_slope, slope_range = True, [0.05, 0.25]
            gravity_observed = False

    cfg = Cfg()
    cfg.env.num_envs = 256
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    first = env.gravity()
    other = make_env(256, seed=SEED)
    explicit = other.draw_gravity(offset_range=(-1.0, 1.0), tilt_range=(0.05, 0.25), observed=False)
    assert torch.equal(first["g"], explicit["g"]) and torch.equal(first["gravity_vec"], explicit["gravity_vec"])
    assert first["g"].unique(dim=0).shape[0] == 256 and first["gravity_vec"].unique(dim=0).shape[0] == 1
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(256, 18, device=DEV))
    assert torch.equal(env.gravity()["g"], first["g"])              # drawn once: resets and steps leave them alone
    env.close(); other.close()


# ------------------------------------------------------------------------------------------------ 8. free flight: a known answer without the oracle
def test_free_flight_differs_from_zero_gravity_by_the_closed_form():
    """Two fp64 envs from the same state - base at z = 5 m, random joint angles and joint / angular velocities - under the same random
    actions, 10 step_physics calls, no contact. Env 0 runs under g = (1.3, -0.7, -6.0), env 1 under g = 0. After n substeps qvel[0:3] must
    differ by n h g and qpos[0:3] by h^2 g n (n + 1) / 2 (semi-implicit Euler), and every other word of qpos and qvel must agree: a
    uniform field exerts no relative force. Tolerance: the project's fp64 state tolerance, 1e-8. (The fp64 emulation of this run holds it,
    tests/test_gravity_emulated.py.)"""
    rng = np.random.default_rng(11)
    g = np.array([1.3, -0.7, -6.0])
    env = make_env(2, dtype=torch.float64, seed=SEED)
    env.reset()
    env.set_gravity(np.stack([g, np.zeros(3)]), [0.0, 0.0, -9.81])
    q, v, w = env.get_state()
    q[:] = q[0]; q[:, 2] = 5.0; q[:, 7:] += rng.uniform(-0.3, 0.3, 18)
    v[:] = 0.0; v[:, 3:] = rng.uniform(-1, 1, 21)
    env.set_state(q, v, np.zeros_like(w))
    dbg = torch.zeros((2, 256), dtype=torch.float64, device=DEV)
    env.set_debug_buffer(dbg)
    nsub, n = int(env.cfg.control.decimation), 0
    for t in range(10):
        env.step_physics(torch.from_numpy(np.tile(rng.uniform(-1, 1, 18).astype(np.float32), (2, 1))))
        n += nsub
        qp, qv, _ = env.get_state()
        assert (dbg.cpu().numpy()[:, DBG_NCON] == 0).all()
        dv, dq = qv[0] - qv[1], qp[0] - qp[1]
        ev = max(np.abs(dv[0:3] - n * H * g).max(), np.abs(dv[3:]).max())
        eq = max(np.abs(dq[0:3] - H * H * g * n * (n + 1) / 2).max(), np.abs(dq[3:]).max())
        print(f"after {n} substeps: velocity error {ev:.2e}, position error {eq:.2e}")
        assert ev < 1e-8 and eq < 1e-8, (t, ev, eq)
    assert env.counters()["bad_state_resets"] == 0
    env.set_debug_buffer(None)
    env.close()


# ------------------------------------------------------------------------------------------------ 9. standing on a slope
def test_standing_on_a_slope_the_observation_shows_the_tilt(G):
    """The fixture's standing states of set 1 (0.2 rad): 20 more zero-action steps in fp32 without a reset; obs[:, 6:9] equals the numpy
    rotation of gravity_vec by the conjugate base quaternion from get_state(), within the fp32 bounds (median < 5e-6, p99 < 1e-4)."""
    N = 8
    sets = np.ones(N, int)
    env = make_env(N, seed=SEED)
    set_gravity(env, G, sets)
    load_state(env, G, "stand", 0, sets)
    vec = G["rows"][1, 4:7]
    errs = []
    for t in range(20):
        obs, _, _, done, _ = env.step(torch.zeros(N, 18))
        assert int(done.sum()) == 0
        q = env.get_state()[0][:, 3:7]
        w, u = q[:, 0:1], -q[:, 1:4]
        tt = 2.0 * np.cross(u, vec)
        want = vec + w * tt + np.cross(u, tt)
        errs.append(np.abs(obs.cpu().numpy()[:, 6:9].astype(np.float64) - want).max(axis=1))
    err = np.stack(errs)
    print(f"obs[6:9] against the rotated gravity_vec: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}; obs x {want[:, 0].mean():.3f}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4
    assert abs(want[:, 0].mean() - 9.81 * np.sin(0.2)) < 0.2      # the policy sees the tilt: about 1.95 m/s^2 along the body's x
    assert env.counters()["bad_state_resets"] == 0
    env.close()
