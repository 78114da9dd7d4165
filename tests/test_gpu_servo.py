"""The servo target model (nm_set_servo and friends, level 5 of the step) on the device, in every stepping path. References: the fp64
fixture of the oracle's rows (tests/golden/servo.npz, make_servo_goldens.py) for what the rows mean, alone (S) and behind the delays of
latency.npz (SL); the numpy recursion of the limiter for servo_state() (bit for bit, no oracle involved); uniform batches for what a
mixed batch must give and the per-step path for the K-step launches (bit for bit); a numpy restatement over oracle.rand_u24 for the draw.
N = 8 throughout (four two-env waves; the rows of the two envs of a wave always differ), N = 7 where a half-empty last wave matters; at
most 10 steps per run."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_latency import scaled
from test_gpu_parity import make_env
from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_push import _actions, _assert_same_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step
from test_servo_host import draw_restated, limiter_restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
POPS = ("drop", "stand")
RECS = ("S", "SL")
H, NSUB = 3, 2
INF = float("inf")
ENVP_SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])
PAYLOADS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])


@pytest.fixture(scope="module")
def G():
    return load_golden("servo.npz")


def default_pos(npdt):
    return np.tile([0.0, np.pi / 5, 0.0], 6).astype(npdt)


def set_rows(env, g, rec, n=None):
    n = env.num_envs if n is None else n
    env.set_servo(g["rate"][:n], g["d_gain"][:n])
    env.set_action_latency(g["delays"][:n] if rec == "SL" else None)


def load_state(env, g, rec, pop, t):
    """Start state, action history AND limited targets of step t; returns the step's (actions, command uniforms)."""
    n = env.num_envs
    pick = lambda k: g[f"{rec}_{pop}_{k}"][t, :n]
    env.set_state(pick("qpos"), pick("qvel"), pick("qw"))
    env.set_buffers(dof_pos=pick("dof_pos"), dof_vel=pick("dof_vel"), actions=pick("act"), commands=pick("cmd"))
    env.episode_length_buf = torch.from_numpy(np.asarray(pick("ep_len"), np.int64)).to(DEV)
    env.set_action_history(pick("hist"))
    env.set_servo_state(pick("lim"))
    return pick("actions"), pick("cmd_u").astype(np.float64)


def step_errors(env, g, rec, pop, t, out):
    n = env.num_envs
    obs, rew, done = out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
    oerr = np.abs(obs.astype(np.float64) - g[f"{rec}_{pop}_obs"][t, :n]).max(axis=1)
    rerr = np.abs(rew.astype(np.float64) - g[f"{rec}_{pop}_rew"][t, :n])
    q, v, _ = env.get_state()
    serr = max(np.abs(q - g[f"{rec}_{pop}_qpos"][t + 1, :n]).max(), np.abs(v - g[f"{rec}_{pop}_qvel"][t + 1, :n]).max())
    lerr = np.abs(env.servo_state() - g[f"{rec}_{pop}_lim"][t + 1, :n]).max()
    return np.maximum(oerr, rerr), serr, lerr, int((done != g[f"{rec}_{pop}_done"][t, :n]).sum())


def forced(env, g, rec, pop, steps):
    errs, serr, lerr, flags = [], 0.0, 0.0, 0
    for t in range(steps):
        a, cu = load_state(env, g, rec, pop, t)
        env.set_command_uniforms(cu)
        e, s, l, f = step_errors(env, g, rec, pop, t, env.step(torch.from_numpy(a)))
        errs.append(e); serr = max(serr, s); lerr = max(lerr, l); flags += f
    return np.stack(errs), serr, lerr, flags


def free(env, g, rec, pop, steps):
    """Free-running from the recording's first state; returns the errors and every step's (obs, rew, done, qpos, qvel, qwarm, L)."""
    errs, serr, lerr, flags, out = [], 0.0, 0.0, 0, []
    n = env.num_envs
    load_state(env, g, rec, pop, 0)
    for t in range(steps):
        env.set_command_uniforms(g[f"{rec}_{pop}_cmd_u"][t, :n].astype(np.float64))
        r = env.step(torch.from_numpy(g[f"{rec}_{pop}_actions"][t, :n]))
        e, s, l, f = step_errors(env, g, rec, pop, t, r)
        errs.append(e); serr = max(serr, s); lerr = max(lerr, l); flags += f
        out.append((r[0].cpu().numpy().copy(), r[2].cpu().numpy().copy(), r[3].cpu().numpy().copy()) + tuple(env.get_state()) + (env.servo_state(),))
    return np.stack(errs), serr, lerr, flags, out


# ------------------------------------------------------------------------------------------------ 1. the kernels vs the oracle's rows
@pytest.mark.parametrize("rec", RECS)
def test_fp64_kernel_matches_the_patched_oracle(G, rec):
    """The fixture's batch under the fixture's rows, alone (S) and behind the delays 0..6, 0 (SL). Teacher-forced single steps and the
    free-running trajectories of both populations: obs / reward < 1e-6, state < 1e-8 (the bounds tests/test_gpu_latency.py asserts for
    the same comparison), no done flag differing; the limited targets after every step are the fixture's bit for bit."""
    env = make_env(8, dtype=torch.float64, seed=SEED)
    set_rows(env, G, rec)
    T = G[f"{rec}_drop_actions"].shape[0]
    for pop in POPS:
        err, serr, lerr, flags = forced(env, G, rec, pop, T)
        print(f"{rec} {pop} forced: max obs/reward error {err.max():.2e}, state {serr:.2e}, limited targets {lerr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8 and lerr == 0.0, (pop, err.max(), serr, lerr)
        err, serr, lerr, flags, _ = free(env, G, rec, pop, T)
        print(f"{rec} {pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}, limited targets {lerr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8 and lerr == 0.0, (pop, "free", err.max(), serr, lerr)
    env.close()


@pytest.mark.parametrize("rec", RECS)
def test_fp32_kernel_is_within_the_fp32_bounds(G, rec):
    """Teacher-forced single steps: median < 5e-6, p99 < 1e-4 (the fp32 emulation of these very states stays inside
    them, tests/test_servo_emulated.py)."""
    env = make_env(8, dtype=torch.float32, seed=SEED)
    set_rows(env, G, rec)
    errs = []
    for pop in POPS:
        err, _, lerr, flags = forced(env, G, rec, pop, G[f"{rec}_{pop}_actions"].shape[0])
        print(f"{rec} {pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, limited targets {lerr:.2e}, done flags differing {flags}")
        assert flags == 0
        assert lerr < 1e-6      # a target below 1 rad in float32: half an ulp of the sum and of the rate each, 6e-8 + 6e-8
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 2. sensitivity
@pytest.mark.parametrize("rec", RECS)
def test_without_the_rows_the_kernel_misses_the_fixture_exactly_where_rows_are_set(G, rec):
    """The comparison of test 1 can fail: with the servo rows cleared (the delays kept) the fp64 kernel leaves the bounds in every env
    with a non-default row and stays inside them in env 0."""
    env = make_env(8, dtype=torch.float64, seed=SEED)
    set_rows(env, G, rec)
    env.set_servo()
    changed = np.isfinite(G["rate"]) | (G["d_gain"] != 0)
    for pop in POPS:
        err, _, _, _ = forced(env, G, rec, pop, G[f"{rec}_{pop}_actions"].shape[0])
        worst = err.max(axis=0)
        assert (worst[changed] > 1e-6).all() and (worst[~changed] < 1e-6).all(), (pop, worst)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. known answer without the oracle
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("N", [8, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_the_limited_targets_are_the_numpy_recursion_bit_for_bit(dtype, N, k):
    """A constant action step input (the targets ramp at their rate, then settle), then random actions: servo_state() after every step
    equals d = T - L; L' = |d| <= rate ? T : L + copysign(rate, d) in the env's dtype - one subtraction, one compare, one add, nothing a
    compiler can contract. With delays k nsub the recursion runs on a_{t-k}. Observation slots 48..65 still show a_t."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    env = make_env(N, dtype=dtype, seed=SEED)
    env.reset()
    rate = np.array([0.03, INF, 0.02, 0.08, 0.04, 0.5, 0.02, 0.08])[:N]
    env.set_servo(rate, 0.05)
    if k:
        env.set_action_latency(k * NSUB)
    lim = env.servo_state().astype(npdt)
    assert not lim.any()      # zero at construction; the feature was off during reset()'s step
    step_in = torch.full((1, N, 18), 0.9, device=DEV) * torch.tensor([1.0, -1.0] * 9, device=DEV)
    acts = torch.cat([step_in.expand(5, N, 18), _actions(5, N)])
    past = [np.zeros((N, 18), np.float32)] * H      # a_{t-1}, a_{t-2}, a_{t-3}: the zero history
    moved_at_rate = settled = 0
    for t in range(acts.shape[0]):
        obs = env.step(acts[t])[0]
        a = scaled(env, acts[t])
        assert torch.equal(obs[:, 48:66], a), (t, "the observation shows the policy's own action")
        a = a.cpu().numpy()
        late = a if k == 0 else past[k - 1]
        target = late.astype(npdt) - default_pos(npdt)
        new = limiter_restated(lim, target, rate.astype(npdt)[:, None])
        assert new.dtype == npdt
        np.testing.assert_array_equal(env.servo_state(), new.astype(np.float64), err_msg=f"step {t}")
        moved_at_rate += int((new != target).sum()); settled += int((new == target)[np.isfinite(rate)].sum())
        lim, past = new, [a] + past[:2]
    assert moved_at_rate > 0 and settled > 0      # both branches of the select
    env.close()


# ------------------------------------------------------------------------------------------------ 4. off = defaults; mixed = uniform
@pytest.mark.parametrize("N", [8, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_never_set_defaults_set_and_set_then_cleared_are_identical(G, dtype, N):
    from nightmare_rl_amd import _lib
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
        s = e.servo()
        assert torch.isinf(s["rate_limit"]).all() and not s["d_gain"].any() and not e.servo_state().any()
    envs[1].set_servo(INF, 0.0)
    envs[2].set_servo(G["rate"][:N], G["d_gain"][:N])
    assert envs[2].servo()["rate_limit"].cpu().tolist() == G["rate"][:N].astype(np.float32 if dtype == torch.float32 else np.float64).tolist()
    # rows the library refuses, before anything of the env changes
    for bad in ((0.0, 0.0), (-0.1, 0.0), (float("nan"), 0.0), (0.1, -0.1), (0.1, INF), (0.1, float("nan"))):
        with pytest.raises(_lib.NightmareHipError, match="nm_set_servo"):
            envs[2].set_servo(*bad)
    with pytest.raises(_lib.NightmareHipError, match="nm_draw_servo"):
        envs[2].draw_servo((0.0, 0.1), None)
    with pytest.raises(ValueError):
        envs[2].set_servo(np.zeros(N + 1) + 0.1, None)
    assert envs[2].servo()["d_gain"].cpu().tolist() == G["d_gain"][:N].astype(np.float32 if dtype == torch.float32 else np.float64).tolist()
    envs[2].set_servo()                                # off again
    assert torch.isinf(envs[2].servo()["rate_limit"]).all() and not envs[2].servo()["d_gain"].any()
    acts = _actions(8, N)
    for s in range(8):
        r = [e.step(acts[s]) for e in envs]
        _assert_same_step(envs[0], envs[1], r[0], r[1], f"default rows, step {s}")
        _assert_same_step(envs[0], envs[2], r[0], r[2], f"set then cleared, step {s}")
    # the limited targets follow the steps taken while the feature is on, and only those
    assert not envs[0].servo_state().any() and not envs[2].servo_state().any()
    npdt = np.float64 if dtype == torch.float64 else np.float32
    want = scaled(envs[1], acts[7]).cpu().numpy().astype(npdt) - default_pos(npdt)
    np.testing.assert_array_equal(envs[1].servo_state(), want.astype(np.float64))
    for e in envs:
        e.close()


@pytest.mark.parametrize("N", [8, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_mixed_batch_equals_the_uniform_batches_bit_for_bit(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL hold e's row and delay. 6 free-running steps of `stand` from the
    SL recording. N = 7: the last wave's second slot is padding, which recomputes env 6 and must store nothing."""
    env = make_env(N, dtype=dtype, seed=SEED)
    set_rows(env, G, "SL")
    mixed = free(env, G, "SL", "stand", 6)[4]
    for e in range(N):
        env.set_servo(float(G["rate"][e]), float(G["d_gain"][e]))
        env.set_action_latency(int(G["delays"][e]))
        uni = free(env, G, "SL", "stand", 6)[4]
        for t, (x, y) in enumerate(zip(mixed, uni)):
            for i, (u, v) in enumerate(zip(x, y)):
                np.testing.assert_array_equal(u[e], v[e], err_msg=f"env {e} step {t} item {i}")
    env.close()


# ------------------------------------------------------------------------------------------------ 5. every stepping path
def _pair(G, N, n=2, everything=False):
    """n envs with the fixture's servo rows (and, with everything, friction / gains, payloads, latency, gravity and pushes as well), reset."""
    envs = [make_env(N, seed=SEED) for _ in range(n)]
    e8 = np.arange(N)
    for e in envs:
        e.reset()
        e.set_servo(G["rate"][:N], G["d_gain"][:N])
        if everything:
            r = ENVP_SETS[(e8 + 1) % 4]
            e.set_env_params(mu=r[:, 0], p_gain=r[:, 1], kv=r[:, 2])
            p = PAYLOADS[(e8 // 2 + e8) % 4]
            e.set_base_payload(p[:, 0], p[:, 1:])
            e.set_action_latency(G["delays"][:N])
            tilt = 0.05 * (1 + e8 % 3)
            e.set_gravity(np.stack([9.81 * np.sin(tilt), np.zeros(N), -9.81 * np.cos(tilt)], axis=1))
            e.set_push(3, 0.5)
    return envs


def _same_targets(ea, eb):
    la, lb = ea.servo_state(), eb.servo_state()
    np.testing.assert_array_equal(la, lb)
    assert la.any()


@pytest.mark.parametrize("everything", [False, True], ids=["servo", "servo+friction+gains+payload+latency+gravity+pushes"])
@pytest.mark.parametrize("N", [8, 7])
def test_tape_equals_the_per_step_path(G, N, everything):
    K = 6
    ea, eb, e0 = _pair(G, N, 3, everything)
    e0.set_servo()
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
    _same_targets(ea, eb)
    assert not e0.servo_state().any()
    changed = (np.isfinite(G["rate"]) | (G["d_gain"] != 0))[:N]
    differs = (rec["obs"][-1] != rec0["obs"][-1]).any(dim=1).cpu().numpy()
    assert differs[changed].all() and not differs[~changed].any()      # the rows were honoured, and by the envs that hold them alone
    for e in (ea, eb, e0):
        e.close()


@pytest.mark.parametrize("everything", [False, True], ids=["servo", "everything"])
@pytest.mark.parametrize("deterministic", [True, False])
def test_play_equals_the_per_step_path(G, deterministic, everything):
    N, K = 8, 6
    ac, fu = _networks()
    ea, eb = _pair(G, N, 2, everything)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    _same_targets(ea, eb)
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("everything", [False, True], ids=["servo", "everything"])
def test_rollout_equals_the_per_step_path(G, everything):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, T, gamma = 8, 6, 0.99
    ac, fu = _networks()
    ea, eb = _pair(G, N, 2, everything)
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
    _same_targets(ea, eb)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 6. the state
def test_a_reset_does_not_clear_the_limited_targets_and_physics_only_leaves_them_alone(G):
    """4-step episodes (cfg.env.episode_length_s = 0.064) with the episode lengths of tests/test_gpu_reset_noise.py: within 10 steps wave 0
    has both envs resetting in the same step, waves 1 and 2 one env at a time, env 6 at steps 4 and 9 - the last step of a 5-step launch.
    The targets after every step are the numpy recursion, which knows nothing of resets; the 5-step tape launch gives the same."""
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    N, K = 8, 10
    eplen = (4, 4, 3, 1, 1, 3, 0, 2)

    def build():
        cfg = NightmareV3Config()
        cfg.env.num_envs, cfg.env.episode_length_s = N, 0.064
        env = NightmareV3Env(cfg, device=DEV, seed=SEED)
        assert int(env.max_episode_length) == 4
        env.reset_idx(None)
        env.episode_length_buf = torch.tensor(eplen, dtype=torch.int64, device=DEV)
        env.set_servo(G["rate"], G["d_gain"])
        return env

    ea, eb = build(), build()
    acts = _actions(K, N)
    lim = np.zeros((N, 18), np.float32)
    resets = np.zeros(N, int)
    for t in range(K):
        done = ea.step(acts[t])[3].cpu().numpy()
        resets += done
        target = scaled(ea, acts[t]).cpu().numpy() - default_pos(np.float32)
        lim = limiter_restated(lim, target, G["rate"].astype(np.float32)[:, None])
        np.testing.assert_array_equal(ea.servo_state(), lim.astype(np.float64), err_msg=f"step {t}")
        if t == 4:
            assert done[6] == 1
    assert (resets == 2).all()
    before = ea.servo_state()
    ea.reset_idx([1, 6])
    ea.reset_idx(None)
    np.testing.assert_array_equal(ea.servo_state(), before)
    ea.step_physics(acts[0])
    np.testing.assert_array_equal(ea.servo_state(), before)
    # the K-step path: two 5-step launches, env 6 resetting at each launch's last step
    for half in (acts[:5], acts[5:]):
        eb.step_tape(half)
    np.testing.assert_array_equal(eb.servo_state(), before)
    back = np.random.default_rng(0).uniform(-1, 1, (N, 18)).astype(np.float32).astype(np.float64)
    ea.set_servo_state(back)
    np.testing.assert_array_equal(ea.servo_state(), back)
    ea.close(); eb.close()


# ------------------------------------------------------------------------------------------------ 7. the config and the draw
def test_upstreams_config_names_switch_the_model_on():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cfg = NightmareV3Config()
    cfg.env.num_envs = 8
    cfg.control.d_gain, cfg.control.action_rate_limit = 0.05, 0.08      # reference envs/nightmare_v3_config.py:37-38, un-commented
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    s = env.servo()
    assert (s["rate_limit"] == np.float32(0.08)).all() and (s["d_gain"] == np.float32(0.05)).all()
    env.reset()      # reset()'s zero-action step runs under the model: the targets head for -default_pos at 0.08 per step
    np.testing.assert_array_equal(env.servo_state(), np.tile(np.float32([0.0, -0.08, 0.0]), (8, 6)).astype(np.float64))
    env.close()
    cfg = NightmareV3Config()
    cfg.env.num_envs = 8
    cfg.control.d_gain = 0.1
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    s = env.servo()
    assert torch.isinf(s["rate_limit"]).all() and (s["d_gain"] == np.float32(0.1)).all()
    env.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_the_draw_is_its_numpy_restatement_and_a_shard_is_a_slice(dtype):
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    npdt = np.float64 if dtype == torch.float64 else np.float32
    lo, hi = [0.02, 0.0], [0.1, 0.2]

    def build(n, offset):
        cfg = NightmareV3Config()
        cfg.env.num_envs = n
        cfg.domain_rand = types.SimpleNamespace(randomize_action_rate_limit=True, action_rate_limit_range=[lo[0], hi[0]],
                                                randomize_d_gain=True, d_gain_range=[lo[1], hi[1]])
        return NightmareV3Env(cfg, device=DEV, seed=SEED, env_id_offset=offset, dtype=dtype)

    whole, shard = build(16, 0), build(8, 8)
    sw, ss = whole.servo(), shard.servo()
    want = draw_restated(SEED, np.arange(16), lo, hi, npdt)
    np.testing.assert_array_equal(sw["rate_limit"].cpu().numpy(), want[:, 0])
    np.testing.assert_array_equal(sw["d_gain"].cpu().numpy(), want[:, 1])
    np.testing.assert_array_equal(ss["rate_limit"].cpu().numpy(), want[8:, 0])      # a shard with env_offset = 8 draws what envs 8.. of the whole got
    np.testing.assert_array_equal(ss["d_gain"].cpu().numpy(), want[8:, 1])
    assert np.unique(want[:, 0]).size > 8 and want[:, 0].min() >= npdt(lo[0]) and want[:, 0].max() <= npdt(hi[0])
    whole.reset()
    for _ in range(3):
        whole.step(torch.zeros(16, 18, device=DEV))
    np.testing.assert_array_equal(whole.servo()["rate_limit"].cpu().numpy(), want[:, 0])      # drawn once: resets and steps leave the rows alone
    # d_gain alone: the rate column is pinned to its default, no limit
    s = whole.draw_servo(None, (0.1, 0.1))
    assert torch.isinf(s["rate_limit"]).all() and (s["d_gain"] == npdt(0.1)).all()
    whole.close(); shard.close()
