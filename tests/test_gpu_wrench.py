"""The external wrench on the base (nm_set_base_wrench, nm_set_wrench_schedule and friends, level 7 of the step) on the device, in every
stepping path. References: the fp64 fixture of the oracle's rows (tests/golden/wrench.npz, make_wrench_goldens.py) for what the rows mean
- the mixed batch gives env e set e % 5, set 3 with its payload, so the two envs of a wave always differ; uniform batches for what a mixed
batch must give and the per-step path for the K-step launches (bit for bit); numpy restatements over oracle.rand_u24 for the schedule and
the draw (tests/wrench_tools.py). N = 8 (four two-env waves) and N = 7 (a half-empty last wave) against the fixture; N = 63 and 1 where
only bits are compared; at most 10 steps per run; schedule interval 3, duration 2 unless a test says otherwise."""
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
from wrench_tools import POPS, draw_restated, mixed, mixed_payload, mixed_wrench, schedule_restated, set_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
INF = float("inf")
IV, DU = 3, 2
MAXF, MAXT = [4.0, 3.0, 2.0], [0.3, 0.2, 0.25]
ENVP_SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])
PAYLOADS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])
DELAYS = np.array([0, 1, 2, 3, 4, 5, 6, 0])
RATE = np.array([INF, 0.03, 0.02, 0.08, 0.04, INF, 0.02, 0.08])
D_GAIN = np.array([0.0, 0.0, 0.05, 0.05, 0.2, 0.2, 0.0, 0.1])
TORQUE = np.array([[INF, INF, INF], [3.2, 3.2, 3.2], [INF, 1.6, INF], [6.4, 0.3, 3.0], [2.0, 2.0, 2.0]])


@pytest.fixture(scope="module")
def G():
    return load_golden("wrench.npz")


def npdt_of(env):
    return np.float64 if env._real == torch.float64 else np.float32


def set_rows(env, g, wrench=True):
    """The mixed batch's rows: set 3's envs carry the payload; wrench False leaves the wrench rows off."""
    n = env.num_envs
    dm, r = mixed_payload(g, n)
    env.set_base_payload(dm, r)
    w = mixed_wrench(g, n)
    if wrench:
        env.set_base_wrench(w[:, :3], w[:, 3:])
    else:
        env.set_base_wrench()


def wrench_of(env):
    """[N,6] (F, tau) as base_wrench() reports them."""
    w = env.base_wrench()
    return torch.cat([w["force"], w["torque"]], dim=1).cpu().numpy()


def load_state(env, g, pop, t):
    """Start state of step t of the mixed batch; returns the step's (actions, command uniforms)."""
    n = env.num_envs
    pick = lambda k: mixed(g, f"{pop}_{k}", t, n)
    env.set_state(pick("qpos"), pick("qvel"), pick("qw"))
    env.set_buffers(dof_pos=pick("dof_pos"), dof_vel=pick("dof_vel"), actions=pick("act"), commands=pick("cmd"))
    env.episode_length_buf = torch.from_numpy(np.asarray(pick("ep_len"), np.int64)).to(DEV)
    return pick("actions"), pick("cmd_u").astype(np.float64)


def step_errors(env, g, pop, t, out):
    n = env.num_envs
    obs, rew, done = out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
    oerr = np.abs(obs.astype(np.float64) - mixed(g, f"{pop}_obs", t, n)).max(axis=1)
    rerr = np.abs(rew.astype(np.float64) - mixed(g, f"{pop}_rew", t, n))
    q, v, _ = env.get_state()
    serr = np.maximum(np.abs(q - mixed(g, f"{pop}_qpos", t + 1, n)).max(axis=1), np.abs(v - mixed(g, f"{pop}_qvel", t + 1, n)).max(axis=1))
    return np.maximum(oerr, rerr), serr, int((done != mixed(g, f"{pop}_done", t, n)).sum())


def forced(env, g, pop, steps):
    errs, serrs, flags = [], [], 0
    for t in range(steps):
        a, cu = load_state(env, g, pop, t)
        env.set_command_uniforms(cu)
        e, s, f = step_errors(env, g, pop, t, env.step(torch.from_numpy(a)))
        errs.append(e); serrs.append(s); flags += f
    return np.stack(errs), np.stack(serrs), flags


def free(env, g, pop, steps, compare=True):
    """Free-running from the recording's first state; returns the errors and every step's (obs, rew, done, qpos, qvel, qwarm)."""
    errs, serrs, flags, out = [], [], 0, []
    n = env.num_envs
    load_state(env, g, pop, 0)
    for t in range(steps):
        env.set_command_uniforms(mixed(g, f"{pop}_cmd_u", t, n).astype(np.float64))
        r = env.step(torch.from_numpy(mixed(g, f"{pop}_actions", t, n)))
        if compare:
            e, s, f = step_errors(env, g, pop, t, r)
            errs.append(e); serrs.append(s); flags += f
        out.append((r[0].cpu().numpy().copy(), r[2].cpu().numpy().copy(), r[3].cpu().numpy().copy()) + tuple(env.get_state()))
    return (np.stack(errs), np.stack(serrs), flags, out) if compare else out


# ------------------------------------------------------------------------------------------------ 1. the kernels vs the oracle's rows
@pytest.mark.parametrize("N", [8, 7])
def test_fp64_kernel_matches_the_patched_oracle(G, N):
    """Teacher-forced single steps and the free-running trajectories of both populations: obs / reward < 1e-6, state < 1e-8 (the
    project's fp64 bounds, tests/test_gpu_parity.py), no done flag differing. The oracle reaches J'[F; tau] through its own jac_point
    and cdof, the kernel through the free joint's closed form. N = 7: the last wave's second slot is padding."""
    env = make_env(N, dtype=torch.float64, seed=SEED)
    set_rows(env, G)
    T = G["drop_actions"].shape[1]
    for pop in POPS:
        err, serr, flags = forced(env, G, pop, T)
        print(f"N={N} {pop} forced: max obs/reward error {err.max():.2e}, state {serr.max():.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr.max() < 1e-8, (pop, err.max(), serr.max())
        err, serr, flags, _ = free(env, G, pop, T)
        print(f"N={N} {pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr.max():.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr.max() < 1e-8, (pop, "free", err.max(), serr.max())
    assert env.step_variant() == "generic"
    env.close()


@pytest.mark.parametrize("N", [8, 7])
def test_fp32_kernel_is_within_the_fp32_bounds(G, N):
    """Teacher-forced single steps: median < 5e-6, p99 < 1e-4."""
    env = make_env(N, dtype=torch.float32, seed=SEED)
    set_rows(env, G)
    errs = []
    for pop in POPS:
        err, _, flags = forced(env, G, pop, G[f"{pop}_actions"].shape[1])
        print(f"N={N} {pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    assert env.step_variant() == "generic"      # the lean kernel is level 0 only
    env.close()


def test_without_the_rows_the_kernel_misses_the_fixture_exactly_where_a_wrench_is_set(G):
    """The comparison of test 1 can fail: with the wrench rows cleared (set 3 keeps its payload) the fp64 kernel leaves the state bound
    in every env of sets 1..4 and stays inside both bounds in those of set 0."""
    env = make_env(8, dtype=torch.float64, seed=SEED)
    set_rows(env, G, wrench=False)
    for pop in POPS:
        err, serr, _ = forced(env, G, pop, G[f"{pop}_actions"].shape[1])
        e, s = err.max(axis=0), serr.max(axis=0)
        loaded = set_of(8) != 0
        assert (s[loaded] > 1e-6).all() and (s[~loaded] < 1e-8).all() and (e[~loaded] < 1e-6).all(), (pop, e, s)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. zero rows = off; 4. mixed = uniform
@pytest.mark.parametrize("N", [63, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_zero_rows_at_level_7_equal_the_kind_switched_off(dtype, N):
    from nightmare_rl_amd import _lib
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
        assert (wrench_of(e) == 0).all()
    envs[1].set_base_wrench(torch.zeros(3), torch.zeros(3))
    rng = np.random.default_rng(3)
    f, t = rng.uniform(-3, 3, (N, 3)), rng.uniform(-0.3, 0.3, (N, 3))
    envs[2].set_base_wrench(f, t)
    npdt = npdt_of(envs[2])
    np.testing.assert_array_equal(wrench_of(envs[2]), np.concatenate([f, t], axis=1).astype(npdt))
    # rows the library refuses, before anything of the env changes
    for bad in ([float("nan"), 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, -INF]):
        with pytest.raises(_lib.NightmareHipError, match="nm_set_base_wrench"):
            envs[2].set_base_wrench(bad, None)
        with pytest.raises(_lib.NightmareHipError, match="nm_set_base_wrench"):
            envs[2].set_base_wrench(None, bad)
    with pytest.raises(ValueError):
        envs[2].set_base_wrench(np.ones((N + 1, 3)))
    np.testing.assert_array_equal(wrench_of(envs[2]), np.concatenate([f, t], axis=1).astype(npdt))
    envs[2].set_base_wrench()                                # off again
    assert (wrench_of(envs[2]) == 0).all()
    acts = _actions(10, N)
    for s in range(10):
        r = [e.step(acts[s]) for e in envs]
        if s == 0:
            assert envs[1].step_variant() == "generic"      # level 7, even under zero rows
            if dtype == torch.float32:
                assert envs[0].step_variant() == "lean" and envs[2].step_variant() == "lean"
        _assert_same_step(envs[0], envs[1], r[0], r[1], f"zero rows, step {s}")
        _assert_same_step(envs[0], envs[2], r[0], r[2], f"set then cleared, step {s}")
    envs[1].set_base_wrench()
    envs[1].step(acts[0])
    if dtype == torch.float32:
        assert envs[1].step_variant() == "lean"      # and lean again after off
    for e in envs:
        e.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_mixed_batch_equals_the_uniform_batches_bit_for_bit(G, dtype):
    """Env e of the mixed batch (N = 63: 31 full waves and a half-empty one) equals env e of the batch whose envs ALL hold e's wrench and
    payload, from the same states: 4 free-running steps of `drop`. And a batch of ONE env equals env 0 of the uniform batch under every set."""
    N = 63
    env, one = make_env(N, dtype=dtype, seed=SEED), make_env(1, dtype=dtype, seed=SEED)
    set_rows(env, G)
    mx = free(env, G, "drop", 4, compare=False)
    for k in range(5):
        w, p = G["sets"][k], G["payload"][k]
        for e in (env, one):
            e.set_base_payload(np.full(e.num_envs, p[0]), np.tile(p[1:], (e.num_envs, 1)))
            e.set_base_wrench(w[:3], w[3:])
        uni = free(env, G, "drop", 4, compare=False)
        single = free(one, G, "drop", 4, compare=False)
        m = set_of(N) == k
        for t, (x, y, z) in enumerate(zip(mx, uni, single)):
            for i, (u, v, ww) in enumerate(zip(x, y, z)):
                np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} step {t} item {i}")
                np.testing.assert_array_equal(ww[0], v[0], err_msg=f"one env, set {k} step {t} item {i}")
    env.close(); one.close()


# ------------------------------------------------------------------------------------------------ 5. the schedule in the per-step path
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_schedule_in_the_per_step_path_is_its_numpy_restatement(dtype):
    """base_wrench() after every one of 8 steps: nothing before step 3, windows open at steps 3 and 6 and close at step 5 (and 8).
    wrench_schedule() reports s. A second env given the state after step 5 and start_step = 5 continues bit for bit."""
    N = 8
    ea, eb = make_env(N, dtype=dtype, seed=SEED), make_env(N, dtype=dtype, seed=SEED)
    npdt = npdt_of(ea)
    ea.reset(); eb.reset()
    ea.set_wrench_schedule(IV, DU, MAXF, MAXT)
    assert ea.wrench_schedule() == (IV, DU, MAXF, MAXT, 0) and (wrench_of(ea) == 0).all()
    want = schedule_restated(SEED, np.arange(N), IV, DU, MAXF + MAXT, npdt, 0, 9)
    acts = _actions(8, N)
    zero = [not w.any() for w in want]
    assert zero == [True, True, True, False, False, True, False, False, True]      # open at 3 and 6, closed at 5 and 8
    for s in range(8):
        if s == 5:      # the checkpoint: the state after step 4 (five steps taken), the schedule's numbers
            eb.set_state(*ea.get_state())
            b = ea.get_buffers()
            eb.set_buffers(dof_pos=b["dof_pos"], dof_vel=b["dof_vel"], actions=b["actions"], commands=b["commands"], episode_sums=b["episode_sums"])
            eb.set_feet_state(*ea.get_feet_state())
            eb.episode_length_buf = ea.episode_length_buf.clone()
            iv, du, mf, mt, st = ea.wrench_schedule()
            assert st == 5
            eb.set_wrench_schedule(iv, du, mf, mt, start_step=st)
            np.testing.assert_array_equal(wrench_of(eb), want[5])      # start_step 5 lies outside a window: zero rows installed
        ra = ea.step(acts[s])
        np.testing.assert_array_equal(wrench_of(ea), want[s], err_msg=f"rows the physics of step {s} read")
        assert ea.wrench_schedule()[4] == s + 1
        if s >= 5:
            rb = eb.step(acts[s])
            np.testing.assert_array_equal(wrench_of(eb), want[s])
            for name, x, y in zip(("qpos", "qvel", "qacc_warmstart"), ea.get_state(), eb.get_state()):
                np.testing.assert_array_equal(x, y, err_msg=f"continued from the checkpoint, step {s} {name}")
            assert torch.equal(ra[2], rb[2])
    # inside a window: start_step 7 installs the draw of window 2
    eb.set_wrench_schedule(IV, DU, MAXF, MAXT, start_step=7)
    np.testing.assert_array_equal(wrench_of(eb), draw_restated(SEED, np.arange(N), 2, MAXF + MAXT, npdt))
    # rows by hand are refused while a schedule is on; interval 0 ends it and zeroes the rows
    from nightmare_rl_amd import _lib
    with pytest.raises(_lib.NightmareHipError, match="a wrench schedule is on"):
        eb.set_base_wrench([1.0, 0.0, 0.0], None)
    eb.set_wrench_schedule(0, 0, 0.0, 0.0)
    assert (wrench_of(eb) == 0).all() and eb.wrench_schedule()[0] == 0
    eb.set_base_wrench([1.0, 0.0, 0.0], None)
    assert (wrench_of(eb)[:, 0] == 1).all()
    ea.close(); eb.close()


def test_duration_equal_to_the_interval_never_zeroes():
    N = 8
    env = make_env(N, seed=SEED)
    env.reset()
    env.set_wrench_schedule(IV, IV, 2.0, 0.1)
    want = schedule_restated(SEED, np.arange(N), IV, IV, [2.0] * 3 + [0.1] * 3, np.float32, 0, 8)
    acts = _actions(8, N)
    for s in range(8):
        env.step(acts[s])
        np.testing.assert_array_equal(wrench_of(env), want[s], err_msg=f"step {s}")
        assert (s < IV) == (not wrench_of(env).any())
    env.close()


# ------------------------------------------------------------------------------------------------ 6. K-step launches; 7. sharding
def _scheduled(N, n=2, offset=0):
    envs = [make_env(N, seed=SEED, env_id_offset=offset) for _ in range(n)]
    for e in envs:
        e.reset()
        e.set_wrench_schedule(IV, DU, MAXF, MAXT)
    return envs


def _assert_same_wrench(ea, eb):
    np.testing.assert_array_equal(wrench_of(ea), wrench_of(eb))
    assert ea.wrench_schedule() == eb.wrench_schedule()


@pytest.mark.parametrize("N", [8, 63])
def test_tape_equals_the_per_step_path(N):
    """K = 7 in one launch, in two launches of 4 + 3 (the window that opens at step 3 straddles the boundary) and step by step: states,
    records, final rows and s."""
    K = 7
    ea, eb, ec, e0 = _scheduled(N, 4)
    e0.set_base_wrench()
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec, rec0, recc = _records(K, N), _records(K, N), _records(K, N)
    oa = ea.step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(eb, acts, bb, ep_idx)
    ec.step_tape(acts[:4], record={k: v[:4] for k, v in recc.items()})
    oc = ec.step_tape(acts[4:], record={k: v[4:] for k, v in recc.items()})
    e0.step_tape(acts, record=rec0)
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
        assert torch.equal(recc[k], per_step[k]), ("4 + 3", k)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    _assert_same_wrench(ea, eb)
    _assert_same_wrench(ec, eb)
    for x, y in zip(ec.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(oc, ob) and ea.wrench_schedule()[4] == K
    np.testing.assert_array_equal(wrench_of(ea), schedule_restated(SEED, np.arange(N), IV, DU, MAXF + MAXT, np.float32, 0, K)[-1])
    # the wrench was honoured: from step 3 on every env differs from the env without it, and no env before
    differs = (rec["obs"] != rec0["obs"]).any(dim=2).cpu().numpy()
    assert not differs[:3].any() and differs[3:5].all()
    for e in (ea, eb, ec, e0):
        e.close()


@pytest.mark.parametrize("N", [8, 63])
@pytest.mark.parametrize("deterministic", [True, False])
def test_play_equals_the_per_step_path(deterministic, N):
    K = 7
    ac, fu = _networks()
    ea, eb = _scheduled(N)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    _assert_same_wrench(ea, eb)
    assert ea.wrench_schedule()[4] == K
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("N", [8, 63])
def test_rollout_equals_the_per_step_path(N):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    T, gamma = 7, 0.99
    ac, fu = _networks()
    ea, eb = _scheduled(N)
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
    _assert_same_wrench(ea, eb)
    assert ea.wrench_schedule()[4] == T
    for e in (ea, eb):
        e.close()


def test_two_shards_of_four_equal_one_population_of_eight():
    """The draw is keyed by the global env id: shards with env_id_offset 0 and 4 equal envs 0..3 and 4..7 of the whole, in the per-step
    path and in a tape launch."""
    K = 7
    (whole,), (lo,), (hi,) = _scheduled(8, 1), _scheduled(4, 1, 0), _scheduled(4, 1, 4)
    (wt,), (lt,), (ht,) = _scheduled(8, 1), _scheduled(4, 1, 0), _scheduled(4, 1, 4)
    acts = _actions(K, 8)
    for s in range(K):
        whole.step(acts[s]); lo.step(acts[s, :4]); hi.step(acts[s, 4:])
        np.testing.assert_array_equal(wrench_of(whole), np.concatenate([wrench_of(lo), wrench_of(hi)]))
    wt.step_tape(acts); lt.step_tape(acts[:, :4].contiguous()); ht.step_tape(acts[:, 4:].contiguous())
    for parts in (zip(whole.get_state(), lo.get_state(), hi.get_state()), zip(wt.get_state(), lt.get_state(), ht.get_state())):
        for w, a, b in parts:
            np.testing.assert_array_equal(w, np.concatenate([a, b]))
    for x, y in zip(whole.get_state(), wt.get_state()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(wrench_of(wt), np.concatenate([wrench_of(lt), wrench_of(ht)]))
    for e in (whole, lo, hi, wt, lt, ht):
        e.close()


# ------------------------------------------------------------------------------------------------ 8. combined kinds
def _everything(n):
    """n envs with 4-step episodes, pools for the six pooled kinds (re-drawn at reset), reset noise and pushes (tests/test_gpu_reset_rows.py),
    the rows of tests/test_gpu_torque_limit.py's combined case, and the wrench schedule."""
    from test_gpu_reset_rows import _env, _start
    N = 8
    e8 = np.arange(N)
    envs = [_env(N, pools=True, noise=True, push=True) for _ in range(n)]
    for e in envs:
        _start(e)
        r = ENVP_SETS[(e8 + 1) % 4]
        e.set_env_params(mu=r[:, 0], p_gain=r[:, 1], kv=r[:, 2])
        p = PAYLOADS[(e8 // 2 + e8) % 4]
        e.set_base_payload(p[:, 0], p[:, 1:])
        e.set_action_latency(DELAYS[e8 % 8])
        tilt = 0.05 * (1 + e8 % 3)
        e.set_gravity(np.stack([9.81 * np.sin(tilt), np.zeros(N), -9.81 * np.cos(tilt)], axis=1))
        e.set_servo(RATE[e8 % 8], D_GAIN[e8 % 8])
        e.set_torque_limit(TORQUE[e8 % 5])
        e.set_wrench_schedule(IV, DU, MAXF, MAXT)
    return envs


def test_all_seven_kinds_pushes_reset_noise_and_pools_together():
    """The per-step path equals the tape, play and rollout launches bit for bit with everything on, over 7 steps in which every env resets
    (its other six rows re-drawn from the pools); the wrench rows after the launches are the schedule's, untouched by the resets."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, K = 8, 7
    ea, eb, ec, ed, ee, ef = _everything(6)
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec = _records(K, N)
    oa = ea.step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(eb, acts, bb, ep_idx)
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
    assert int(per_step["done"].sum(dim=0).min()) >= 1      # every env reset at least once
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    _assert_same_wrench(ea, eb)
    want = schedule_restated(11, np.arange(N), IV, DU, MAXF + MAXT, np.float32, 0, K)[-1]      # tests/test_gpu_reset_rows.py's seed
    np.testing.assert_array_equal(wrench_of(ea), want)
    np.testing.assert_array_equal(wrench_of(eb), want)
    # a reset that re-draws the other six leaves the wrench rows alone
    before = [x.clone() for x in (ea.torque_limit(), ea.gravity()["g"])]
    ea.reset_idx([1, 6])
    np.testing.assert_array_equal(wrench_of(ea), want)
    assert any(not torch.equal(x, y) for x, y in zip(before, (ea.torque_limit(), ea.gravity()["g"])))
    # play
    ac, fu = _networks()
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    bc, bd = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oc = ec.policy_play(K, fu.flat, deterministic=False, seed=77, iter_dev=it, stats=_stats(bc, ep_idx))
    od, _ = _play_step_by_step(ed, fu, K, False, 77, it, bd, ep_idx)
    _assert_same_env(ec, ed, oc, od)
    _assert_same_books(bc, bd)
    _assert_same_wrench(ec, ed)
    # rollout (an env may time out once per rollout: 4 steps)
    T, gamma = 4, 0.99
    be, bf = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    se, sf = _storage(N, T), _storage(N, T)
    it3 = torch.tensor([3], dtype=torch.int64, device=DEV)
    oe = ee.policy_rollout(T, fu.flat, 99, it3, se, gamma, be["cur_ret"], be["cur_len"], be["fin"], ep=(ep_idx, be["ep_acc"]))
    o = ef.get_observations()
    for s in range(T):
        act = ef.policy_act(fu.flat, o, 99, it3, s, sf)
        o, _, rew, done, infos = ef.step(act)
        _record(L, ef, sf, s, gamma, bf["cur_ret"], bf["cur_len"], bf["fin"], ep_idx, bf["ep_acc"])
    torch.cuda.synchronize()
    for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(se, name), getattr(sf, name)), name
    _assert_same_env(ee, ef, oe, o)
    _assert_same_wrench(ee, ef)
    for e in (ea, eb, ec, ed, ee, ef):
        e.close()


# ------------------------------------------------------------------------------------------------ 9. physics-only launches
def test_physics_only_launches_honour_the_rows_and_leave_s_alone(G):
    """nm_step_physics is physics: under a constant wrench it leaves the state a launch without it reaches, and equals a second env under
    the same rows bit for bit (level 7 with the run-time skip of latency and the servo row). Under a schedule it leaves s and the rows alone."""
    ea, eb, e0 = (make_env(8, seed=SEED) for _ in range(3))
    acts = _actions(3, 8)
    for e in (ea, eb, e0):
        e.reset()
    w = mixed_wrench(G, 8)
    w[set_of(8) == 0] = [1.0, 1.0, 1.0, 0.1, 0.1, 0.1]
    ea.set_base_wrench(w[:, :3], w[:, 3:]); eb.set_base_wrench(w[:, :3], w[:, 3:])
    eb.set_servo(0.05, 0.1); eb.set_action_latency(3)      # ignored by a physics-only launch
    for t in range(3):
        for e in (ea, eb, e0):
            e.step_physics(acts[t])
    qa, qb, q0 = ea.get_state()[0], eb.get_state()[0], e0.get_state()[0]
    np.testing.assert_array_equal(qa, qb)
    assert (np.abs(qa - q0).max(axis=1) > 1e-6).all()
    e0.set_wrench_schedule(IV, DU, MAXF, MAXT, start_step=3)
    rows = wrench_of(e0)
    assert rows.any()
    for t in range(3):
        e0.step_physics(acts[t])
    assert e0.wrench_schedule()[4] == 3
    np.testing.assert_array_equal(wrench_of(e0), rows)
    for e in (ea, eb, e0):
        e.close()


# ------------------------------------------------------------------------------------------------ the config
def test_the_config_names_switch_the_schedule_on():
    import types
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cfg = NightmareV3Config()
    cfg.env.num_envs = 8
    cfg.domain_rand = types.SimpleNamespace(external_wrench=True, wrench_interval_s=0.048, wrench_duration_s=0.032, max_wrench_force=[4.0, 3.0, 2.0],
                                            max_wrench_torque=0.25)
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    assert env.wrench_schedule() == (3, 2, [4.0, 3.0, 2.0], [0.25] * 3, 0) and env.wrench_interval == 3
    env.reset()
    for s in range(4):
        env.step(torch.zeros(8, 18, device=DEV))
    assert env.step_variant() == "generic"
    np.testing.assert_array_equal(wrench_of(env), draw_restated(SEED, np.arange(8), 1, [4.0, 3.0, 2.0] + [0.25] * 3, np.float32))
    env.close()
