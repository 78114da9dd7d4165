"""Per-env actuation latency (nm_set_action_latency and friends) on the device, in every stepping path. References: the fp64 fixture of
the oracle's rows (tests/golden/latency.npz, make_latency_goldens.py) for what a delay means; uniform batches for what a mixed batch must
give (bit for bit: every env is independent); an undelayed env fed the shifted action sequence for whole-step delays (bit for bit, no
oracle involved); the per-step path for the K-step launches (bit for bit); a numpy restatement over oracle.rand_u24 for the draw.
N = 8 throughout (four two-env waves; the fixture's delays 0..6, 0 put two different switch substeps into a wave), N = 7 where a
half-empty last wave matters; at most 10 steps per run."""
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
from test_latency_host import draw_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
POPS = ("drop", "stand")
H, NSUB = 3, 2
ENVP_SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])
PAYLOADS = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.03, 0.0, 0.04], [-0.3, 0.0, 0.0, 0.0], [1.0, -0.05, 0.02, 0.05]])


@pytest.fixture(scope="module")
def G():
    return load_golden("latency.npz")


def scaled(env, a):
    """a_t: the action after scale and clip, float32, as the load stage computes it (one rounding of the product, then the clip)."""
    c = float(env.cfg.normalization.clip_actions)
    return torch.clamp(a.to(torch.float32) * np.float32(env.cfg.control.action_scale), -c, c)


def load_state(env, g, pop, t):
    """Start state AND action history of step t, env e of the fixture; returns the step's (actions, command uniforms)."""
    n = env.num_envs
    pick = lambda k: g[f"{pop}_{k}"][t, :n]
    env.set_state(pick("qpos"), pick("qvel"), pick("qw"))
    env.set_buffers(dof_pos=pick("dof_pos"), dof_vel=pick("dof_vel"), actions=pick("act"), commands=pick("cmd"))
    env.episode_length_buf = torch.from_numpy(np.asarray(pick("ep_len"), np.int64)).to(DEV)
    env.set_action_history(pick("hist"))
    return pick("actions"), pick("cmd_u").astype(np.float64)


def step_errors(env, g, pop, t, out):
    n = env.num_envs
    obs, rew, done = out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
    oerr = np.abs(obs.astype(np.float64) - g[f"{pop}_obs"][t, :n]).max(axis=1)
    rerr = np.abs(rew.astype(np.float64) - g[f"{pop}_rew"][t, :n])
    q, v, _ = env.get_state()
    serr = max(np.abs(q - g[f"{pop}_qpos"][t + 1, :n]).max(), np.abs(v - g[f"{pop}_qvel"][t + 1, :n]).max())
    return np.maximum(oerr, rerr), serr, int((done != g[f"{pop}_done"][t, :n]).sum())


def forced(env, g, pop, steps):
    errs, serr, flags = [], 0.0, 0
    for t in range(steps):
        a, cu = load_state(env, g, pop, t)
        env.set_command_uniforms(cu)
        e, s, f = step_errors(env, g, pop, t, env.step(torch.from_numpy(a)))
        errs.append(e); serr = max(serr, s); flags += f
        np.testing.assert_array_equal(env.action_history().cpu().numpy(), g[f"{pop}_hist"][t + 1, :env.num_envs])
    return np.stack(errs), serr, flags


def free(env, g, pop, steps):
    """Free-running from the fixture's first state; returns the errors and every step's (obs, rew, done, qpos, qvel, qwarm)."""
    errs, serr, flags, out = [], 0.0, 0, []
    n = env.num_envs
    load_state(env, g, pop, 0)
    for t in range(steps):
        env.set_command_uniforms(g[f"{pop}_cmd_u"][t, :n].astype(np.float64))
        r = env.step(torch.from_numpy(g[f"{pop}_actions"][t, :n]))
        e, s, f = step_errors(env, g, pop, t, r)
        errs.append(e); serr = max(serr, s); flags += f
        out.append((r[0].cpu().numpy().copy(), r[2].cpu().numpy().copy(), r[3].cpu().numpy().copy()) + tuple(env.get_state()))
    out.append((env.action_history().cpu().numpy(),))
    return np.stack(errs), serr, flags, out


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the oracle's rows
def test_fp64_kernel_matches_the_patched_oracle(G):
    """The fixture's batch, delays 0..6 and 0. Teacher-forced single steps and the free-running trajectories of both populations:
    obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py), no done flag differing; the history
    after every step is the fixture's."""
    env = make_env(8, dtype=torch.float64, seed=SEED)
    env.set_action_latency(G["delays"])
    T = G["drop_actions"].shape[0]
    for pop in POPS:
        err, serr, flags = forced(env, G, pop, T)
        print(f"{pop} forced: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, err.max(), serr)
        err, serr, flags, out = free(env, G, pop, T)
        print(f"{pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, "free", err.max(), serr)
        np.testing.assert_array_equal(out[-1][0], G[f"{pop}_hist"][T])
    env.close()


# ------------------------------------------------------------------------------------------------ 2. fp32 kernel vs the fixture
def test_fp32_kernel_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps: median < 5e-6, p99 < 1e-4 (the bounds tests/test_gpu_env_params.py applies to the fp32 kernel; the fp32
    emulation of these very states stays inside them, tests/test_latency_emulated.py)."""
    env = make_env(8, dtype=torch.float32, seed=SEED)
    env.set_action_latency(G["delays"])
    errs = []
    for pop in POPS:
        err, _, flags = forced(env, G, pop, G[f"{pop}_actions"].shape[0])
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 3. mixed batch = uniform batches
@pytest.mark.parametrize("N", [8, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_mixed_batch_equals_the_seven_uniform_batches_bit_for_bit(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL hold e's delay (same states, histories and actions): what
    differs between the runs is only when e's wave neighbour switches its command. 8 free-running steps per population. N = 7: the last
    wave's second slot is padding, which recomputes env 6 and must store nothing."""
    delays = G["delays"][:N]
    env = make_env(N, dtype=dtype, seed=SEED)
    env.set_action_latency(delays)
    dbg = torch.zeros((N, 256), dtype=dtype, device=DEV)
    env.set_debug_buffer(dbg)
    mixed = {pop: free(env, G, pop, 8)[3] for pop in POPS}
    ntog = int(dbg.cpu().numpy()[0::2, 156].sum())      # the last step's two-env constraint passes (nm_core.h env_debug, word 156)
    env.set_debug_buffer(None)
    if dtype == torch.float32:
        assert ntog >= 1
    for d in range(7):
        env.set_action_latency(np.full(N, d, np.int32))
        m = delays == d
        assert m.any()
        for pop in POPS:
            uni = free(env, G, pop, 8)[3]
            for t, (x, y) in enumerate(zip(mixed[pop], uni)):
                for i, (u, v) in enumerate(zip(x, y)):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"delay {d} {pop} step {t} item {i}")
    env.close()


# ------------------------------------------------------------------------------------------------ 4. off = delay 0
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_never_set_all_zero_and_set_then_cleared_are_bit_identical(G, dtype):
    from nightmare_rl_amd import _lib
    N = 8
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
        assert e.action_latency().dtype == torch.int32 and not e.action_latency().any() and not e.action_history().any()
    envs[1].set_action_latency(0)
    envs[2].set_action_latency(G["delays"])
    assert envs[2].action_latency().cpu().tolist() == G["delays"].tolist()
    # delays the library refuses, before anything of the env changes
    for bad in (7, -1, [0, 1, 2, 3, 4, 5, 6, 9]):
        with pytest.raises(_lib.NightmareHipError, match="nm_set_action_latency"):
            envs[2].set_action_latency(bad)
    with pytest.raises(_lib.NightmareHipError, match="nm_draw_action_latency"):
        envs[2].draw_action_latency(0, 7)
    with pytest.raises(ValueError):
        envs[2].set_action_latency(1.5)
    assert envs[2].action_latency().cpu().tolist() == G["delays"].tolist()
    envs[2].set_action_latency()                                # off again
    assert not envs[2].action_latency().any()
    acts = _actions(8, N)
    for s in range(8):
        r = [e.step(acts[s]) for e in envs]
        _assert_same_step(envs[0], envs[1], r[0], r[1], f"all-zero delays, step {s}")
        _assert_same_step(envs[0], envs[2], r[0], r[2], f"set then cleared, step {s}")
    # the history follows the steps taken while the feature is on, and only those
    assert not envs[0].action_history().any() and not envs[2].action_history().any()
    assert torch.equal(envs[1].action_history()[:, 0], scaled(envs[1], acts[7]))
    # a physics-only launch ignores latency and leaves the history alone
    envs[2].set_action_latency(G["delays"])
    for e in (envs[0], envs[2]):
        e.step_physics(acts[0])
    for x, y in zip(envs[0].get_state(), envs[2].get_state()):
        np.testing.assert_array_equal(x, y)
    assert not envs[2].action_history().any()
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. shift identity
@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_whole_step_delay_is_the_undelayed_env_fed_the_shifted_sequence(k):
    """No oracle: an env with delay k nsub whose history holds a_{-1}, a_{-2}, ... and which is fed a_t aims its servos where a delay-0
    env fed a_{t-k} does - qpos, qvel and qacc_warmstart are bit-equal after every step. Its observation slots 48..65 still show a_t."""
    N, K = 8, 8
    seq = _actions(K + k, N)                    # seq[t] is what the undelayed env is fed at step t; the delayed one is fed seq[t + k]
    ea, eb = make_env(N, seed=SEED), make_env(N, seed=SEED)
    for e in (ea, eb):
        e.reset()
    ea.set_action_latency(k * NSUB)
    hist = torch.zeros(N, H, 18, device=DEV)
    for j in range(k):
        hist[:, j] = scaled(ea, seq[k - 1 - j])
    ea.set_action_history(hist)
    for t in range(K):
        ra, rb = ea.step(seq[t + k]), eb.step(seq[t])
        torch.cuda.synchronize()
        for name, x, y in zip(("qpos", "qvel", "qacc_warmstart"), ea.get_state(), eb.get_state()):
            np.testing.assert_array_equal(x, y, err_msg=f"k {k} step {t} {name}")
        assert torch.equal(ra[3], rb[3]), (k, t, "done")
        assert torch.equal(ra[0][:, 48:66], scaled(ea, seq[t + k])), (k, t, "the observation shows the policy's own action")
        assert torch.equal(ra[0][:, :48], rb[0][:, :48]), (k, t, "the rest of the observation is the physics'")
    assert not torch.equal(ea.step(seq[0])[0][:, :48], eb.step(seq[0])[0][:, :48])      # ... and the delay is not a no-op: same action now, different targets
    ea.close(); eb.close()


# ------------------------------------------------------------------------------------------------ 6. every stepping path
def _pair(G, N, n=2, rows=False):
    """n envs with the fixture's delays (and, with rows, friction / gains and payloads mixed over the envs as well), reset."""
    envs = [make_env(N, seed=SEED) for _ in range(n)]
    e8 = np.arange(N)
    for e in envs:
        e.reset()
        e.set_action_latency(G["delays"][:N])
        if rows:
            r = ENVP_SETS[(e8 + 1) % 4]
            e.set_env_params(mu=r[:, 0], p_gain=r[:, 1], kv=r[:, 2])
            p = PAYLOADS[(e8 // 2 + e8) % 4]
            e.set_base_payload(p[:, 0], p[:, 1:])
    return envs


def _same_history(ea, eb, last_actions):
    ha, hb = ea.action_history(), eb.action_history()
    assert torch.equal(ha, hb)
    assert ha.any() and torch.equal(ha[:, 0], scaled(ea, last_actions))


@pytest.mark.parametrize("rows", [False, True], ids=["latency", "latency+friction+gains+payload"])
@pytest.mark.parametrize("N", [8, 7])
def test_tape_with_latency_equals_the_per_step_path(G, N, rows):
    K = 6
    ea, eb, e0 = _pair(G, N, 3, rows)
    e0.set_action_latency()
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
    _same_history(ea, eb, acts[K - 1])
    differs = (rec["obs"][-1] != rec0["obs"][-1]).any(dim=1).cpu().numpy()
    assert differs[G["delays"][:N] > 0].all() and not differs[G["delays"][:N] == 0].any()      # the delays were honoured, and by the delayed envs alone
    for e in (ea, eb, e0):
        e.close()


@pytest.mark.parametrize("deterministic", [True, False])
def test_play_with_latency_equals_the_per_step_path(G, deterministic):
    N, K = 8, 6
    ac, fu = _networks()
    ea, eb = _pair(G, N)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    ha, hb = ea.action_history(), eb.action_history()
    assert torch.equal(ha, hb) and ha.any()
    np.testing.assert_array_equal(ha[:, 0].cpu().numpy(), ea.get_buffers()["actions"].astype(np.float32))
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("rows", [False, True], ids=["latency", "latency+friction+gains+payload"])
def test_rollout_with_latency_equals_the_per_step_path(G, rows):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, T, gamma = 8, 6, 0.99
    ac, fu = _networks()
    ea, eb = _pair(G, N, 2, rows)
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
    _same_history(ea, eb, sa.actions[T - 1])
    for e in (ea, eb):
        e.close()


def test_latency_alone_equals_latency_with_default_rows_set_explicitly(G):
    """Latency alone (the host then supplies default friction / gain and body rows) equals latency with those rows set at their defaults,
    and switching the other features off again while latency stays on restores it. fp32, bit for bit, 8 free-running steps."""
    N = 8
    ea, eb = make_env(N, seed=SEED), make_env(N, seed=SEED)
    for e in (ea, eb):
        e.set_action_latency(G["delays"])
    eb.set_env_params(mu=ENVP_SETS[1, 0], p_gain=ENVP_SETS[1, 1], kv=ENVP_SETS[1, 2])
    eb.set_base_payload(0.5, [0.03, 0.0, 0.04])
    eb.set_env_params()
    eb.set_base_payload()
    assert eb.action_latency().cpu().tolist() == G["delays"].tolist()
    xa, xb = free(ea, G, "stand", 8)[3], free(eb, G, "stand", 8)[3]
    eb.set_env_params(mu=ENVP_SETS[0, 0], p_gain=ENVP_SETS[0, 1], kv=ENVP_SETS[0, 2])
    eb.set_base_payload(0.0)
    xc = free(eb, G, "stand", 8)[3]
    for x, y, z in zip(xa, xb, xc):
        for u, v, w in zip(x, y, z):
            np.testing.assert_array_equal(u, v)
            np.testing.assert_array_equal(u, w)
    ea.close(); eb.close()


# ------------------------------------------------------------------------------------------------ 8. the draw
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_the_draw_is_its_numpy_restatement_and_lies_in_range(dtype):
    whole = make_env(16, dtype=dtype, seed=SEED)
    shard = make_env(8, dtype=dtype, seed=SEED, env_id_offset=8)
    dw, ds = whole.draw_action_latency(0, 6).cpu().numpy(), shard.draw_action_latency(0, 6).cpu().numpy()
    np.testing.assert_array_equal(dw, draw_np(SEED, 0, 16, 0, 6))
    np.testing.assert_array_equal(ds, dw[8:])                      # a shard with env_offset = 8 draws what envs 8.. of the whole got
    assert dw.min() >= 0 and dw.max() <= 6 and np.unique(dw).size >= 4
    np.testing.assert_array_equal(whole.draw_action_latency(2, 5).cpu().numpy(), draw_np(SEED, 0, 16, 2, 5))
    assert whole.action_latency().min() >= 2 and whole.action_latency().max() <= 5
    np.testing.assert_array_equal(whole.draw_action_latency(3, 3).cpu().numpy(), np.full(16, 3))
    whole.close(); shard.close()


# ------------------------------------------------------------------------------------------------ 9. the config
def test_cfg_domain_rand_draws_at_construction():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

    class Cfg(NightmareV3Config):
        class domain_rand:
            randomize_action_latency, action_latency_range = True, [1, 6]

    cfg = Cfg()
    cfg.env.num_envs = 64
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    d = env.action_latency().cpu().numpy()
    np.testing.assert_array_equal(d, draw_np(SEED, 0, 64, 1, 6))
    assert d.min() >= 1 and d.max() <= 6 and np.unique(d).size == 6
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(64, 18, device=DEV))
    np.testing.assert_array_equal(env.action_latency().cpu().numpy(), d)          # drawn once: resets and steps leave the delays alone
    env.close()


# ------------------------------------------------------------------------------------------------ 10. the history
def test_the_history_is_the_last_three_scaled_and_clipped_actions_and_survives_a_reset(G):
    N, K = 8, 5
    env = make_env(N, seed=SEED)
    env.reset()
    env.set_action_latency(G["delays"])
    acts = _actions(K, N) * 40.0            # well past the clip in many joints
    for t in range(K):
        env.step(acts[t])
        h = env.action_history()
        for j in range(H):
            want = scaled(env, acts[t - j]) if t - j >= 0 else torch.zeros(N, 18, device=DEV)
            assert torch.equal(h[:, j], want), (t, j)
    assert float(h.abs().max()) == float(env.cfg.normalization.clip_actions)
    env.reset_idx(None)
    assert torch.equal(env.action_history(), h)                  # reset_idx leaves the actions alone upstream, and so does this
    env.reset_idx([1, 6])
    assert torch.equal(env.action_history(), h)
    env.reset()                                                  # reset() is reset_idx and ONE step under zero actions: a step like any other
    h2 = env.action_history()
    assert torch.equal(h2[:, 1:], h[:, :2]) and not h2[:, 0].any()
    back = torch.rand(N, H, 18, device=DEV)
    env.set_action_history(back)
    assert torch.equal(env.action_history(), back)
    env.close()
