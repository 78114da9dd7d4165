"""Per-env friction and servo gains (nm_set_env_params / nm_get_env_params / nm_draw_env_params) on the device, in every stepping path.
References: the fp64 fixture of the oracle's rows (tests/golden/env_params.npz, make_envparam_goldens.py) for what the values mean;
uniform batches for what a mixed batch must give (bit for bit: every env is independent); the per-step path for the K-step launches
(bit for bit); a numpy restatement over oracle.rand_u24 for the draw."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import make_env
from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_push import _actions, _assert_same_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
POPS = ("drop", "stand", "belly")
ENVP_KEY = 0x454E5650          # nm::kEnvParamKey (nm_core.h)
DBG_NTOG, DBG_NCON = 156, 160  # words of an env's debug row (nm_core.h env_debug)
DEFAULT = (1.0, 20.0, 0.8)


@pytest.fixture(scope="module")
def G():
    return load_golden("env_params.npz")


def set_of(n):
    """Parameter set of env e: neighbours in a wave (2w, 2w + 1) always hold different sets, and every set meets both slots."""
    e = np.arange(n)
    return (e + e // 4) % 4


def set_rows(env, rows):
    rows = np.asarray(rows, np.float64)
    env.set_env_params(mu=rows[:, 0], p_gain=rows[:, 1], kv=rows[:, 2])


def load_state(env, g, pop, t, sets):
    """Start state of step t: env e takes env e % 8 of the trajectory of set sets[e]. Returns the step's (actions, command uniforms)."""
    ev = np.arange(len(sets)) % 8
    pick = lambda k: g[f"{pop}_{k}"][sets, t, ev]
    env.set_state(pick("qpos"), pick("qvel"), pick("qw"))
    env.set_buffers(dof_pos=pick("dof_pos"), dof_vel=pick("dof_vel"), actions=pick("act"), commands=pick("cmd"))
    env.episode_length_buf = torch.from_numpy(np.asarray(pick("ep_len"), np.int64)).to(DEV)
    return g[f"{pop}_actions"][sets, t, ev], g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64)


def step_errors(env, g, pop, t, sets, out):
    ev = np.arange(len(sets)) % 8
    obs, rew, done = out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
    oerr = np.abs(obs.astype(np.float64) - g[f"{pop}_obs"][sets, t, ev]).max(axis=1)
    rerr = np.abs(rew.astype(np.float64) - g[f"{pop}_rew"][sets, t, ev])
    q, v, _ = env.get_state()
    serr = max(np.abs(q - g[f"{pop}_qpos"][sets, t + 1, ev]).max(), np.abs(v - g[f"{pop}_qvel"][sets, t + 1, ev]).max())
    return np.maximum(oerr, rerr), serr, int((done != g[f"{pop}_done"][sets, t, ev]).sum())


def forced(env, g, pop, sets, steps):
    errs, serr, flags = [], 0.0, 0
    for t in range(steps):
        a, cu = load_state(env, g, pop, t, sets)
        env.set_command_uniforms(cu)
        e, s, f = step_errors(env, g, pop, t, sets, env.step(torch.from_numpy(a)))
        errs.append(e); serr = max(serr, s); flags += f
    return np.stack(errs), serr, flags


def free(env, g, pop, sets, steps):
    errs, serr, flags = [], 0.0, 0
    load_state(env, g, pop, 0, sets)
    ev = np.arange(len(sets)) % 8
    for t in range(steps):
        env.set_command_uniforms(g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64))
        e, s, f = step_errors(env, g, pop, t, sets, env.step(torch.from_numpy(g[f"{pop}_actions"][sets, t, ev])))
        errs.append(e); serr = max(serr, s); flags += f
    return np.stack(errs), serr, flags


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the variant oracles
def test_fp64_kernel_with_mixed_sets_matches_the_variant_oracles(G):
    """N = 32, the four sets mixed over the envs. Teacher-forced single steps and the free-running trajectories of all three populations:
    obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_rows(env, G["sets"][sets])
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
    """Env e of the mixed batch equals env e of the batch whose envs ALL hold e's set (same states, same actions): what differs between the
    runs is only what e's wave neighbour carries. 8 steps per population. N = 63: 31 full waves and a half-filled one; the fp32 kernel
    must have taken both envs of a wave through ONE constraint pass, and both kernels the matrix-free layout, at least once."""
    sets = set_of(N) if N > 1 else np.array([3])
    mixed = make_env(N, dtype=dtype, seed=SEED)
    set_rows(mixed, G["sets"][sets])
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
        set_rows(uni, np.repeat(G["sets"][k][None], N, axis=0))
        m = sets == k
        for pop in POPS:
            other, _, _ = _run8(uni, G, pop, sets)
            for t, (x, y) in enumerate(zip(runs[pop], other)):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart"), x, y):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} {pop} step {t} {name}")
        uni.close()


# ------------------------------------------------------------------------------------------------ 3. fp32 kernel vs the fixture
def test_fp32_kernel_with_mixed_sets_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps, N = 32: median < 5e-6, p99 < 1e-4 (the bounds of tests/test_gpu_parity.py for the fp32 kernel on
    contact-rich states; the fp32 emulation of these very states stays inside them, tests/test_env_params_emulated.py)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float32, seed=SEED)
    set_rows(env, G["sets"][sets])
    errs = []
    for pop in POPS:
        err, _, flags = forced(env, G, pop, sets, G[f"{pop}_actions"].shape[1])
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 4. off = never set
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_never_set_identity_values_and_set_then_cleared_are_bit_identical(dtype):
    N = 63
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
    envs[1].set_env_params(mu=DEFAULT[0], p_gain=torch.full((N,), DEFAULT[1]), kv=np.full(N, DEFAULT[2]))
    envs[2].set_env_params(mu=0.3, p_gain=11.0, kv=1.4)
    envs[2].set_env_params()                                            # all None: off again
    for e in envs:
        p = e.env_params()
        for k, v in zip(("mu", "p_gain", "kv"), DEFAULT):
            assert p[k].dtype == dtype and torch.equal(p[k].cpu(), torch.full((N,), v, dtype=dtype)), k
    acts = _actions(8, N)
    for s in range(8):
        r = [e.step(acts[s]) for e in envs]
        _assert_same_step(envs[0], envs[1], r[0], r[1], f"identity values, step {s}")
        _assert_same_step(envs[0], envs[2], r[0], r[2], f"set then cleared, step {s}")
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. every stepping path
def _mixed_pair(N, n=2):
    envs = [make_env(N, seed=SEED) for _ in range(n)]
    rows = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])[set_of(N)]
    for e in envs:
        e.reset()
        set_rows(e, rows)
    return envs


@pytest.mark.parametrize("N", [63, 130])
def test_tape_with_parameters_equals_the_per_step_path(N):
    K = 8
    ea, eb, e0 = _mixed_pair(N, 3)
    e0.set_env_params()
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
    assert not torch.equal(rec["obs"][-1], rec0["obs"][-1])               # the parameters were honoured
    assert torch.equal(rec["obs"][-1][0::16], rec0["obs"][-1][0::16])     # ... and env 0, 16, ... hold the default set: untouched
    for e in (ea, eb, e0):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
@pytest.mark.parametrize("deterministic", [True, False])
def test_play_with_parameters_equals_the_per_step_path(N, deterministic):
    K = 8
    ac, fu = _networks()
    ea, eb = _mixed_pair(N)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
def test_rollout_with_parameters_equals_the_per_step_path(N):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    T, gamma = 8, 0.99
    ac, fu = _networks()
    ea, eb = _mixed_pair(N)
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
    for e in (ea, eb):
        e.close()


def test_physics_only_steps_honour_friction_and_damping(G):
    """nm_step_physics from the fixture's standing states: an env with another mu, and one with another kv, ends elsewhere than with the
    defaults; an env whose row holds the defaults ends exactly where the feature-off run does."""
    N = 8
    sets = np.zeros(N, int)
    envs = [make_env(N, seed=SEED) for _ in range(2)]
    rows = np.repeat(np.array([DEFAULT]), N, axis=0)
    rows[1, 0], rows[2, 2] = 0.4, 1.4
    set_rows(envs[1], rows)
    for e in envs:
        a, _ = load_state(e, G, "stand", 0, sets)
        a = a.copy(); a[:] = 0.5                                    # a servo command away from the pose: the feet push on the floor
        for _ in range(4):
            e.step_physics(torch.from_numpy(a))
    (q0, v0, _), (q1, v1, _) = envs[0].get_state(), envs[1].get_state()
    keep = np.array([0, 3, 4, 5, 6, 7])
    np.testing.assert_array_equal(q0[keep], q1[keep]); np.testing.assert_array_equal(v0[keep], v1[keep])
    print("largest velocity difference: mu 0.4 vs 1.0", np.abs(v0[1] - v1[1]).max(), " kv 1.4 vs 0.8", np.abs(v0[2] - v1[2]).max())
    assert np.abs(v0[1] - v1[1]).max() > 1e-6 and np.abs(v0[2] - v1[2]).max() > 1e-6          # far above fp32 rounding of O(1) velocities' differences: a changed solve, not noise
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 6. sharding
def test_drawn_values_and_results_do_not_depend_on_sharding():
    whole = make_env(128, seed=SEED)
    parts = [make_env(64, seed=SEED, env_id_offset=off) for off in (0, 64)]
    for e in [whole] + parts:
        e.reset()
        e.draw_env_params(friction_range=(0.4, 1.6), stiffness_multiplier_range=(0.7, 1.3), damping_multiplier_range=(0.6, 1.4))
    pw, pp = whole.env_params(), [p.env_params() for p in parts]
    for k in ("mu", "p_gain", "kv"):
        assert torch.equal(pw[k], torch.cat([p[k] for p in pp])), k
        assert pw[k].unique().numel() > 100
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


# ------------------------------------------------------------------------------------------------ 7. the draw
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_draw_is_its_numpy_restatement_uniform_in_range_and_round_trips(dtype):
    from oracle import oracle as orc
    N, npdt = 4096, (np.float64 if dtype == torch.float64 else np.float32)
    env = make_env(N, dtype=dtype, seed=SEED, env_id_offset=1000)
    fr, st, da = (0.4, 1.6), (0.7, 1.3), (1.0, 1.0)
    env.draw_env_params(friction_range=fr, stiffness_multiplier_range=st, damping_multiplier_range=da)
    got = {k: v.cpu().numpy() for k, v in env.env_params().items()}
    lo = np.array([fr[0], 20.0 * st[0], 0.8 * da[0]]).astype(npdt)
    hi = np.array([fr[1], 20.0 * st[1], 0.8 * da[1]]).astype(npdt)
    for c, k in enumerate(("mu", "p_gain", "kv")):
        u = np.array([orc.rand_u24((SEED + ENVP_KEY) & (2 ** 64 - 1), 1000 + e, c) for e in range(N)]).astype(npdt)      # 24 bits: exact
        want = lo[c] + u * (hi[c] - lo[c])                       # numpy rounds the product, then the sum: what the kernel is written to do
        assert want.dtype == npdt
        np.testing.assert_array_equal(got[k], want, err_msg=k)
        w = float(hi[c]) - float(lo[c])
        if w == 0:
            assert (got[k] == lo[c]).all()                       # lo == hi pins the value
            continue
        assert got[k].min() >= lo[c] and got[k].max() <= hi[c]
        assert got[k].max() - got[k].min() > 0.99 * w            # 4096 draws reach within 1 % of both ends (misses with probability < 1e-8)
        bound = 5 * w / math.sqrt(12 * N)                        # five standard deviations of the mean of N draws from U[lo, hi)
        mean = got[k].astype(np.float64).mean()
        print(k, "mean", mean, "expected", (float(lo[c]) + float(hi[c])) / 2, "bound", bound)
        assert abs(mean - (float(lo[c]) + float(hi[c])) / 2) < bound, k
    # nm_set_env_params -> nm_get_env_params round trip, a None column = its default
    mu = torch.linspace(0.3, 1.7, N, dtype=dtype, device=DEV)
    env.set_env_params(mu=mu, kv=0.65)
    p = env.env_params()
    assert torch.equal(p["mu"], mu) and (p["p_gain"] == 20.0).all() and torch.equal(p["kv"], torch.full((N,), 0.65, dtype=dtype, device=DEV))
    # refusals name the column; a refused call changes nothing
    from nightmare_rl_amd import _lib
    for kw, word in ((dict(friction_range=(0.0, 1.0)), "mu"), (dict(friction_range=(1.2, 1.0)), "mu"),
                     (dict(stiffness_multiplier_range=(-0.5, 1.0)), "p_gain"), (dict(damping_multiplier_range=(0.5, float("inf"))), "kv")):
        with pytest.raises(_lib.NightmareHipError, match=word):
            env.draw_env_params(**kw)
    assert torch.equal(env.env_params()["mu"], mu)
    env.close()


def test_cfg_domain_rand_draws_at_construction():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

    class Cfg(NightmareV3Config):
        class domain_rand:
            randomize_friction, friction_range = True, [0.5, 1.25]
            randomize_gains, stiffness_multiplier_range = True, [0.9, 1.1]

    cfg = Cfg()
    cfg.env.num_envs = 256
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    p = env.env_params()
    assert 0.5 <= float(p["mu"].min()) and float(p["mu"].max()) <= 1.25 and float(p["mu"].max() - p["mu"].min()) > 0.375      # half the range
    assert 18.0 <= float(p["p_gain"].min()) and float(p["p_gain"].max()) <= 22.0 and float(p["p_gain"].max() - p["p_gain"].min()) > 2.0
    assert (p["kv"] == torch.tensor(0.8, dtype=torch.float32)).all()
    first = {k: v.clone() for k, v in p.items()}
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(256, 18, device=DEV))
    for k, v in env.env_params().items():
        assert torch.equal(v, first[k]), k                          # drawn once: resets and steps leave them alone
    env.close()


# ------------------------------------------------------------------------------------------------ 8. physical sanity
def test_more_damping_leaves_a_free_swing_slower():
    """Robot held high (no contact within 20 steps: it falls 0.5 m of the 5 m), every joint swinging at 2 rad/s, identical (zero) actions and
    p_gain = 0 in both envs: the servo command is then zero and the actuator force is -kv * qvel, viscous damping and nothing else (in free
    fall gravity exerts no torque about the joints). The joint velocities decay like exp(-kv t / inertia), so after the 20 steps the sum of
    their squares is smaller at kv = 1.6 than at kv = 0.4. (The fp32 emulation of this very run: 7.3e-6 against 1.2e-4.)"""
    env = make_env(2, seed=SEED)
    env.reset()
    q, v, w = env.get_state()
    q[:, 2] = 5.0
    q[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
    q[:, 7:] = 0.0
    v[:] = 0.0
    v[:, 6:] = 2.0
    env.set_state(q, v, np.zeros_like(w))
    env.set_buffers(dof_pos=q[:, 7:], dof_vel=v[:, 6:], actions=np.zeros((2, 18)))
    env.set_env_params(p_gain=0.0, kv=torch.tensor([0.4, 1.6]))
    a = torch.zeros((2, 18))
    for _ in range(20):
        env.step(a)
    q, v, _ = env.get_state()
    assert q[:, 2].min() > 4.0
    e = (v[:, 6:] ** 2).sum(axis=1)
    print("sum of squared joint velocities: kv 0.4 ->", e[0], " kv 1.6 ->", e[1])
    assert e[1] < e[0]
    assert env.counters()["bad_state_resets"] == 0
    env.close()


def test_a_shoved_robot_travels_farther_on_a_slippery_floor(G):
    """Standing robots (the fixture's settled states), base velocity set to 0.5 m/s along x, servos holding the pose: Coulomb friction
    decelerates a sliding body by about mu g, so the distance covered before it stops falls with mu. 25 steps (0.4 s): at mu = 1.5 the feet
    grip (0.5 m/s is gone within v / (mu g) = 0.03 s), at mu = 0.3 they slide for 0.17 s."""
    N = 2
    sets = np.zeros(N, int)
    env = make_env(N, seed=SEED)
    a, _ = load_state(env, G, "stand", 0, sets)
    q, v, w = env.get_state()
    q[1] = q[0]; v[1] = v[0]; w[1] = w[0]
    v[:, 0:2] = 0.0
    v[:, 0] = 0.5
    y0 = q[:, 0].copy()
    env.set_state(q, v, w)
    b = env.get_buffers()
    env.set_buffers(dof_pos=np.repeat(b["dof_pos"][:1], N, axis=0), dof_vel=np.repeat(b["dof_vel"][:1], N, axis=0), actions=np.zeros((N, 18)))
    env.set_env_params(mu=torch.tensor([0.3, 1.5]))
    for _ in range(25):
        env.step(torch.zeros(N, 18))
    q, _, _ = env.get_state()
    d = q[:, 0] - y0
    print("travel along x: mu 0.3 ->", d[0], " mu 1.5 ->", d[1])
    assert d[0] > d[1] and d[0] > 0
    env.close()
