"""The one-launch rollout with privileged critic observations (nm_rollout_priv; csrc/nm_rollout_kernels.h under NM_ROLLOUT_PRIV): the wave
policy on [N, 89] rows against torch, the launch against the step-by-step path BIT FOR BIT with every randomisation that moves a privileged
column inside a launch, the level-0 defaults, the refusals, and the runner's opt-in."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import make_env
from test_gpu_privileged_obs import _env, _tilt
from test_gpu_rollout import _record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOBS, NROW = 66, 89
RESET_RANGES = ((0.0, 0.03), (-0.15, 0.15), (-0.3, 0.3), (-0.3, 0.3), (-0.8, 0.8))


def _networks(activation="elu", seed=5, std=0.8):
    from nightmare_rl_amd.rl import ActorCritic
    from nightmare_rl_amd.rl.fused import FusedUpdate
    torch.manual_seed(seed)
    ac = ActorCritic(NOBS, NROW, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation=activation, init_noise_std=std).to(DEV)
    with torch.no_grad():      # biases away from zero, distinct std per action: nothing in the packing may hide behind a default
        for m in list(ac.actor) + list(ac.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
        ac.std.mul_(torch.linspace(0.6, 1.4, 18, device=DEV))
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), DEV, lr=1e-3)
    assert not fu.has_fast_path
    return ac, fu


def _storage(N, T, nobs=NOBS, nrow=NROW):
    from nightmare_rl_amd.rl import RolloutStorage
    return RolloutStorage(N, T, [nobs], [nrow], [18], DEV)


# ------------------------------------------------------------------------------------------------ (a) the wave policy on wide rows
@pytest.mark.parametrize("activation", ["elu", "tanh"])
def test_wave_policy_reads_the_wide_row_and_the_actor_only_its_prefix(activation):
    """nm_rollout_act_priv at N = 37 (odd: the last wave is half empty) against torch actor(rows[:, :66]) / critic(rows), with the tolerances
    of the symmetric wave policy in tests/test_gpu_rollout.py (exact-f32 FMA chains in another order: mu 2e-5 abs + 1e-5 rel, value 3e-5);
    both stored rows are the inputs bit for bit; other privileged columns leave mu, actions and log-probabilities bit-identical - the
    actor's packed layer-0 weights are exact zeros there - and change the values."""
    N = 37
    ac, fu = _networks(activation)
    env = _env(N)
    st = _storage(N, 3)
    torch.manual_seed(21)
    rows = torch.randn(N, NROW, device=DEV) * 2.0
    it = torch.tensor([7], dtype=torch.int64, device=DEV)
    a = env.policy_act(fu.flat, rows, 1234, it, 2, st, activation=activation)
    with torch.no_grad():
        mu, v = ac.actor(rows[:, :NOBS]), ac.critic(rows).squeeze(-1)
    print(f"{activation}: max |mu - torch| {float((st.mu[2] - mu).abs().max()):.3e}, max |value - torch| {float((st.values[2].squeeze(-1) - v).abs().max()):.3e}")
    torch.testing.assert_close(st.mu[2], mu, atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(st.values[2].squeeze(-1), v, atol=3e-5, rtol=1e-5)
    assert torch.equal(st.sigma[2], ac.std.detach().expand(N, 18)) and a.data_ptr() == st.actions[2].data_ptr()
    assert torch.equal(st.observations[2], rows[:, :NOBS]) and torch.equal(st.privileged_observations[2], rows)
    lp = torch.distributions.Normal(st.mu[2], st.sigma[2]).log_prob(st.actions[2]).sum(-1)
    torch.testing.assert_close(st.actions_log_prob[2].squeeze(-1), lp, atol=2e-4, rtol=1e-5)
    assert float(st.mu[0].abs().sum() + st.mu[1].abs().sum() + st.privileged_observations[:2].abs().sum()) == 0.0      # only row 2 was written
    first = {k: getattr(st, k)[2].clone() for k in ("mu", "actions", "actions_log_prob", "values")}
    other = rows.clone()
    other[:, NOBS:] = torch.randn(N, NROW - NOBS, device=DEV) * 3.0
    env.policy_act(fu.flat, other, 1234, it, 2, st, activation=activation)
    for k in ("mu", "actions", "actions_log_prob"):
        assert torch.equal(getattr(st, k)[2], first[k]), k
    assert not torch.equal(st.values[2], first["values"])
    assert torch.equal(st.observations[2], rows[:, :NOBS]) and torch.equal(st.privileged_observations[2], other)
    env.close()


# ------------------------------------------------------------------------------------------------ (b), (c) one launch = step by step
def _randomised(N):
    """Pools that every reset re-draws friction / gains, payload and latency from, a wrench schedule (interval 3, duration 2), reset noise
    and a push every 4 steps: each moves a privileged column, or the state behind one, inside a launch."""
    e = _env(N, seed=11)
    k = np.arange(5, dtype=np.float64)
    e.set_reset_pool("env_params", mu=0.5 + 0.15 * k, p_gain=15.0 + 2.5 * k, kv=0.6 + 0.1 * k)
    e.set_reset_pool("base_payload", dm=0.2 * k - 0.3, r=np.stack([0.01 * k, -0.005 * k, 0.01 + 0.005 * k], axis=1))
    e.set_reset_pool("action_latency", substeps=np.array([0, 1, 2, 3, 5]))
    e.reset()
    e.set_wrench_schedule(3, 2, [4.0, 3.0, 2.0], [0.3, 0.2, 0.25])
    e.set_reset_noise(RESET_RANGES)
    e.set_push(4, 0.3)
    return e


def _plain(N):
    e = _env(N, seed=11)
    e.reset()
    return e


def _compare(N, T, make, rollouts, activation="elu"):
    """A: policy_rollout. B: T x [policy_act on the env's wide row, step(), nm_ppo_record]. Returns A's storages (one per rollout) and dones."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    ac, fu = _networks(activation)
    gamma = 0.99
    envs = [make(N), make(N)]
    n_to = max(N // 2, 4)
    for e in envs:
        torch.manual_seed(3)
        e.episode_length_buf = torch.randint(0, 1200, (N,), device=DEV, dtype=torch.int64)
        e.episode_length_buf[:n_to] = 1249 - torch.arange(n_to, device=DEV) % (rollouts * T)      # time-outs spread over all rollouts
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    ep_idx = torch.tensor([envs[0]._stat_names.index(k[4:]) for k in sorted(envs[0].extras["episode"])], dtype=torch.int32, device=DEV)
    book = [dict(cur_ret=torch.zeros(N, device=DEV), cur_len=torch.zeros(N, device=DEV), fin=torch.zeros(3, device=DEV), ep_acc=torch.zeros(ep_idx.numel(), device=DEV))
            for _ in envs]
    kept = []
    for r in range(rollouts):
        it.fill_(3 + r)
        for e in envs:
            _tilt(e, N - 2 - r)          # laid on its side: its next step terminates it
        sa, sb = _storage(N, T), _storage(N, T)
        ea, ba = envs[0], book[0]
        obs_before, priv_before = ea.get_observations(), ea.get_privileged_observations()
        keep_o, keep_p = obs_before.clone(), priv_before.clone()
        lv = torch.full((N,), float("nan"), device=DEV)
        oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]), last_values=lv, activation=activation)
        pa = ea.get_privileged_observations()
        assert torch.equal(obs_before, keep_o) and torch.equal(priv_before, keep_p) and pa.data_ptr() != priv_before.data_ptr()      # double-buffered
        eb, bb = envs[1], book[1]
        rows = eb.get_privileged_observations()
        for s in range(T):
            act = eb.policy_act(fu.flat, rows, 99, it, s, sb, activation=activation)
            o, rows, rew, done, infos = eb.step(act)
            _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
        torch.cuda.synchronize()
        for name in ("observations", "privileged_observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
            x, y = getattr(sa, name), getattr(sb, name)
            assert torch.equal(x, y), (r, name, float((x.float() - y.float()).abs().max()), (x != y).any(dim=-1).nonzero()[:6].tolist())
        assert torch.equal(sa.privileged_observations[..., :NOBS], sa.observations)
        assert torch.equal(oa, o) and torch.equal(pa, rows) and torch.equal(pa[:, :NOBS], oa)
        assert torch.equal(ea.rew_buf, eb.rew_buf) and torch.equal(ea.reset_buf, eb.reset_buf)
        tmp = _storage(N, 1)
        eb.policy_act(fu.flat, rows, 99, it, 0, tmp, activation=activation)
        assert torch.equal(lv, tmp.values[0].view(-1))
        with torch.no_grad():
            torch.testing.assert_close(lv, ac.critic(rows).view(-1), atol=3e-5, rtol=1e-5)
        assert torch.equal(ea.episode_length_buf, eb.episode_length_buf) and torch.equal(ea.time_out_buf, eb.time_out_buf)
        for x, y in zip(ea.get_state(), eb.get_state()):
            np.testing.assert_array_equal(x, y)
        ba_, bb_ = ea.get_buffers(), eb.get_buffers()
        for k in ba_:
            np.testing.assert_array_equal(ba_[k], bb_[k], err_msg=k)
        assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
        torch.testing.assert_close(ba["fin"], bb["fin"], atol=1e-3, rtol=1e-5)                 # float atomics: order of the additions differs
        assert ba["fin"][2] == bb["fin"][2]
        torch.testing.assert_close(ba["ep_acc"], bb["ep_acc"], atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(ea._ep_stats, eb._ep_stats, atol=1e-6, rtol=1e-4)
        assert ea.counters() == eb.counters() and ea.common_step_counter == eb.common_step_counter
        # the per-env rows and the schedules' counters behind the privileged columns
        pa_, pb_ = ea.env_params(), eb.env_params()
        assert all(torch.equal(pa_[k], pb_[k]) for k in pa_)
        assert torch.equal(ea.base_payload()["rows"], eb.base_payload()["rows"]) and torch.equal(ea.action_latency(), eb.action_latency())
        wa, wb = ea.base_wrench(), eb.base_wrench()
        assert all(torch.equal(wa[k], wb[k]) for k in wa) and ea.wrench_schedule() == eb.wrench_schedule() and ea.push_state() == eb.push_state()
        np.testing.assert_array_equal(ea.reset_row_counts(), eb.reset_row_counts())
        np.testing.assert_array_equal(ea.reset_noise_state()[2], eb.reset_noise_state()[2])
        kept.append(sa)
    # and the env keeps working through plain step() afterwards, identically on both sides
    a = torch.rand(N, 18, device=DEV) * 2 - 1
    for _ in range(2):
        ra, rb = envs[0].step(a), envs[1].step(a)
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]) and torch.equal(ra[3], rb[3])
    for e in envs:
        e.close()
    return kept


def test_one_launch_equals_step_by_step_bit_for_bit_with_everything_moving():
    """N = 63 (half a wave empty), T = 12, two rollouts back to back, level 7: pools on friction / gains, payload and latency, a wrench
    schedule (3, 2), reset noise, a push every 4 steps; time-outs inside both rollouts and one env per rollout laid on its side. Every
    storage array, the returned rows, last_values, state, buffers, counters and the rows behind the columns must be equal; the float-atomic
    sums to the symmetric test's tolerances. The privileged columns are NOT constant inside a launch: a friction column changes behind a
    reset, and the wrench columns open and close."""
    N, T = 63, 12
    kept = _compare(N, T, _randomised, 2)
    for r, st in enumerate(kept):
        pv, dones = st.privileged_observations, st.dones.squeeze(-1) > 0
        assert int(dones[:-1].sum()) >= 3, r                                          # resets whose next row is still inside this launch
        assert dones[:, N - 2 - r].any(), r                                           # the tilted env terminated
        mu = pv[..., NOBS + 0]
        moved_at_reset = (mu[1:] != mu[:-1]) & dones[:-1]
        assert moved_at_reset.any(), r                                                # a row from the pool shows up in the step after the reset
        assert not ((mu[1:] != mu[:-1]) & ~dones[:-1]).any(), r                       # and nowhere else
        w = pv[..., NOBS + 16:NOBS + 22]
        on = (w != 0).any(dim=-1)
        assert (on[1:] & ~on[:-1]).any() and (~on[1:] & on[:-1]).any(), r             # a window opens and a window closes inside the launch
        assert (pv[1:, :, NOBS + 22] != pv[:-1, :, NOBS + 22]).any()                  # base height follows the state


def test_level_0_files_the_default_columns():
    """The same comparison with no per-env rows set (level 0, no block: the gather takes its default branch), N = 8, T = 6: the storage
    holds the default columns of the table in DESIGN 6.20 - mu, 1, 1, zeros, gravity (0, 0, -1), zeros - and the base height."""
    N, T = 8, 6
    st = _compare(N, T, _plain, 1)[0]
    probe = _plain(N)
    d = probe.privileged_defaults()
    probe.close()
    want = np.zeros(22, np.float32)
    want[[0, 1, 2, 10]] = [d["mu"], 1.0, 1.0, -1.0]
    got = st.privileged_observations.cpu().numpy()
    assert np.array_equal(got[..., NOBS:NOBS + 22], np.broadcast_to(want, (T, N, 22)))
    h = got[..., NOBS + 22]
    assert (h > 0.02).all() and (h < 0.5).all() and len(np.unique(h)) > N


# ------------------------------------------------------------------------------------------------ (d) refusals
def test_refusals():
    from nightmare_rl_amd import _lib
    L = _lib.load()
    ac, fu = _networks()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    N = 8
    env64 = _env(N, dtype=torch.float64)
    env64.reset()
    with pytest.raises(_lib.NightmareHipError, match="fp32"):
        env64.policy_rollout(4, fu.flat, 0, it, _storage(N, 4), 0.99, z(N), z(N), z(3))
    with pytest.raises(_lib.NightmareHipError, match="fp32"):
        env64.policy_act(fu.flat, z(N, NROW), 0, it, 0, _storage(N, 4))
    env = _env(N)
    env.reset()
    for nobs, nrow in ((NOBS, 90), (NOBS, NOBS), (64, NROW)):      # storage widths other than 66 / 89
        with pytest.raises(ValueError, match="privileged"):
            env.policy_rollout(4, fu.flat, 0, it, _storage(N, 4, nobs, nrow), 0.99, z(N), z(N), z(3))
        with pytest.raises(ValueError, match="privileged"):
            env.policy_act(fu.flat, z(N, nrow), 0, it, 0, _storage(N, 4, nobs, nrow))
    with pytest.raises(ValueError, match="privileged"):                # a 66-wide row for a privileged storage
        env.policy_act(fu.flat, z(N, NOBS), 0, it, 0, _storage(N, 4))
    off = make_env(N)                                                  # the privileged switch off
    off.reset()
    with pytest.raises(ValueError, match="privileged"):
        off.policy_rollout(4, fu.flat, 0, it, _storage(N, 4), 0.99, z(N), z(N), z(3))
    with pytest.raises(ValueError, match="privileged"):
        off.policy_act(fu.flat, z(N, NROW), 0, it, 0, _storage(N, 4))
    with pytest.raises(_lib.NightmareHipError, match="more steps than an episode"):
        env.policy_rollout(2000, fu.flat, 0, it, _storage(N, 2000), 0.99, z(N), z(N), z(3))
    # NULL privileged pointers, at the C entry point
    a, pa = _lib.NmRolloutArgs(), _lib.NmRolloutPrivArgs()
    a.steps = 4
    assert L.nm_rollout_priv(env._h, C.byref(a), C.byref(pa), 0, None) != 0 and "NULL privileged pointer" in L.nm_last_error().decode()
    assert L.nm_rollout_priv(env._h, C.byref(a), None, 0, None) != 0
    assert L.nm_rollout_priv(env._h, C.byref(a), C.byref(pa), 99, None) != 0 and "activation" in L.nm_last_error().decode()
    # nothing above launched anything: the env steps on
    o, p, *_ = env.step(z(N, 18))
    assert torch.isfinite(p).all() and torch.equal(p[:, :NOBS], o)
    for e in (env64, env, off):
        e.close()


# ------------------------------------------------------------------------------------------------ (e) the runner
def test_runner_collects_through_the_privileged_one_launch_rollout():
    """OnPolicyRunner with cfg['runner']['privileged_rollout'] = True on an env with privileged observations and two randomisation kinds on,
    N = 64, 8 steps per env, 2 iterations: the mode says one launch, the generic fused update trains both networks, and what the launch filed
    is the prefix / row pair with the drawn friction in column 66."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3ConfigPPO
    from nightmare_rl_amd.rl import OnPolicyRunner

    class domain_rand:
        randomize_friction, friction_range = True, (0.5, 1.25)
        randomize_base_mass, added_mass_range = True, (-0.2, 0.4)

    cfg = class_to_dict(NightmareV3ConfigPPO())
    cfg["runner"]["num_steps_per_env"] = 8
    cfg["runner"]["save_interval"] = 1000
    cfg["runner"]["privileged_rollout"] = True
    torch.manual_seed(0)
    env = _env(64, seed=1, domain_rand=domain_rand)
    r = OnPolicyRunner(env, cfg, log_dir=None, device=DEV)
    alg = r.alg
    assert alg.fused.asymmetric and alg.fused.update is None and not alg.fused_update.has_fast_path
    assert alg.fused.can_rollout(env) is False and alg.fused.can_rollout_privileged(env) is True
    before = alg.fused_update.flat.clone()
    r.learn(2, init_at_random_ep_len=True)
    assert r.rollout_mode.startswith("one launch") and r.rollout_mode == "one launch (nm_rollout, privileged)" and len(r.history) == 2
    assert np.isfinite([h["value_loss"] for h in r.history]).all() and np.isfinite([h["surrogate_loss"] for h in r.history]).all()
    after = alg.fused_update.flat
    n_actor = sum(p.numel() for p in alg.actor_critic.actor.parameters())
    assert torch.isfinite(after).all()
    assert not torch.equal(before[:n_actor], after[:n_actor]) and not torch.equal(before[n_actor:-18], after[n_actor:-18])
    st = alg.storage
    assert st.privileged_observations.shape == (8, 64, NROW) and torch.equal(st.privileged_observations[..., :NOBS], st.observations)
    mu = st.privileged_observations[..., NOBS]
    assert float(mu.min()) >= 0.5 and float(mu.max()) < 1.25 and float(mu.std()) > 0.0
    assert torch.equal(env.get_privileged_observations()[:, :NOBS], env.get_observations())
    env.close()
