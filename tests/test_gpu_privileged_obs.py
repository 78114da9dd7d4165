"""Privileged critic observations (cfg.env.privileged_obs; envs/privileged.py, csrc/nm_priv_obs.h) and the asymmetric actor-critic on the
hand-written PPO kernels: the row against the env's own getters, off is off, the generic mini-batch kernel against torch autograd + Adam
with the critic fed the wide row and the actor its prefix, the collector, the runner end to end, and the refusal of a wider actor."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import _ppo_reference_losses, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = 23
DIVIDED = [1, 2, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21]      # columns that hold a quotient; the others are copies or differences
COPIED = [c for c in range(NP) if c not in DIVIDED]


def _env(N, dtype=torch.float32, seed=3, priv=True, noise=False, domain_rand=None):
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cls = NightmareV3Config
    if priv:
        class cls(NightmareV3Config):
            class env(NightmareV3Config.env):
                privileged_obs = True
    cfg = cls()
    cfg.env.num_envs, cfg.noise.add_noise = N, noise
    if domain_rand is not None:
        cfg.domain_rand = domain_rand
    return NightmareV3Env(cfg, device=DEV, seed=seed, dtype=dtype)


def _reference(env, obs):
    """privileged_reference fed from the env's getters and qpos, all read now."""
    from nightmare_rl_amd.envs.privileged import privileged_reference
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    ep, sv, wr = env.env_params(), env.servo(), env.base_wrench()
    return privileged_reference(obs.cpu().numpy(), env.privileged_defaults(), base_height=env.get_state()[0][:, 2], mu=n(ep["mu"]), p_gain=n(ep["p_gain"]),
                                kv=n(ep["kv"]), body_rows=n(env.base_payload()["rows"]), latency=n(env.action_latency()), g=n(env.gravity()["g"]),
                                rate_limit=n(sv["rate_limit"]), d_gain=n(sv["d_gain"]), torque_limit=n(env.torque_limit()), force=n(wr["force"]),
                                torque=n(wr["torque"]))


def _check_row(env, obs, priv):
    assert priv.shape == (env.num_envs, 89) and priv.dtype == torch.float32 and priv.is_cuda
    assert torch.equal(priv[:, :66], obs) and obs is env.obs_buf and priv is env.get_privileged_observations()
    got, want = priv.cpu().numpy()[:, 66:], _reference(env, obs)[:, 66:]
    np.testing.assert_array_equal(got[:, COPIED], want[:, COPIED])
    np.testing.assert_allclose(got[:, DIVIDED], want[:, DIVIDED], rtol=1e-6, atol=0)
    return got


def _tilt(env, e):
    """Lay env e on its side (74 degrees about x, as tests/golden/make_goldens.py's tilted starts): its next step terminates it."""
    qpos, qvel, qw = env.get_state()
    qpos[e, 2], qpos[e, 3], qpos[e, 4:7] = 0.25, np.cos(0.65), [np.sin(0.65), 0.0, 0.0]
    env.set_state(qpos, qvel, qw)


def _set_every_kind(env, N):
    i = np.arange(N, dtype=np.float64)
    inf_env = 1
    rate = 0.05 + 0.03 * i
    rate[inf_env] = np.inf
    lim = 3.0 + 0.5 * i[:, None] + np.array([0.0, 1.0, 2.0])
    lim[inf_env] = np.inf
    env.set_env_params(mu=0.6 + 0.1 * i, p_gain=16.0 + 2.0 * i, kv=0.7 + 0.05 * i)
    env.set_base_payload(dm=0.1 * i - 0.15, r=np.stack([0.01 * i, -0.005 * i, 0.02 + 0.0 * i], axis=1))
    env.set_action_latency(np.arange(N) % 7)
    th = 0.03 * (i + 1)
    env.set_gravity(np.stack([9.81 * np.sin(th), 0.1 * i, -9.81 * np.cos(th)], axis=1))
    env.set_servo(rate_limit=rate, d_gain=0.01 * i)
    env.set_torque_limit(lim)
    env.set_base_wrench(force=np.stack([1.0 * i, -0.5 * i, 0.25 * i], axis=1), torque=np.stack([0.1 * i, 0.2 + 0.0 * i, -0.05 * i], axis=1))
    return inf_env


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kinds", ["every-kind", "no-kind"])
def test_row_against_the_getters(dtype, kinds):
    """N = 5 (the last workgroup's run is short, the last wave of the step half empty), 4 steps of fixed actions, env 3 laid on its side
    before step 2 so that it resets there. After every step: columns 0..65 are obs_buf bit for bit, columns 66.. equal privileged_reference
    fed from the getters and qpos read at the same point (copied and subtracted columns exactly, quotients to rtol 1e-6: one rounding
    to float32 of a float64 quotient on both sides, 6e-8, plus the summation order of the model's total mass), and the tensor step t
    returned is untouched by step t + 1."""
    N = 5
    env = _env(N, dtype)
    assert env.num_privileged_obs == 89 and env.privileged_obs_has_obs_prefix is True
    inf_env = _set_every_kind(env, N) if kinds == "every-kind" else None
    obs, priv = env.reset()
    _check_row(env, obs, priv)
    rng = np.random.default_rng(0)
    actions = torch.from_numpy(rng.uniform(-1, 1, (4, N, 18)).astype(np.float32)).to(DEV)
    for t in range(4):
        if t == 2:
            _tilt(env, 3)
        before, before_obs = priv, priv.clone()
        obs, priv, _, done, _ = env.step(actions[t])
        got = _check_row(env, obs, priv)
        assert priv.data_ptr() != before.data_ptr() and torch.equal(before, before_obs)
        assert int(done[3]) == (1 if t == 2 else 0)
        if t == 2:
            assert got[3, 22] == np.float32(0.15)       # the height AFTER the in-step reset (qpos0's), not the 0.25 it was laid at
        if kinds == "every-kind":
            assert got[inf_env, 11] == 0.0 and (got[inf_env, 13:16] == 0.0).all() and (got[0, 13:16] > 0).all()
            assert len(set(got[:, 0])) == N and len(set(got[:, 7])) == N and (got[1:, 16] > 0).all() and (got[:, 19:22] != 0).any()
        else:
            d = env.privileged_defaults()
            want = np.zeros(22, np.float32)
            want[[0, 1, 2, 10]] = [d["mu"], 1.0, 1.0, -1.0]
            assert np.array_equal(got[:, :22], np.broadcast_to(want, (N, 22)))
    env.close()


def test_row_of_the_resetting_step_shows_rows_from_the_pools():
    """resample_on_reset with a pool of 3 rows per kind: the rows re-drawn by an in-step reset appear in the row that step returns (the
    rows the next step runs under), each kind's columns being those of one pool row."""
    from nightmare_rl_amd.envs.privileged import privileged_reference
    N = 5
    env = _env(N)
    k = np.arange(3, dtype=np.float64)
    body = dict(dm=0.2 * k - 0.1, r=np.stack([0.01 * k, 0.0 * k, 0.01 + 0.01 * k], axis=1))
    g = np.stack([0.5 * k, 0.0 * k, -9.81 + 0.1 * k], axis=1)
    env.set_reset_pool("env_params", mu=0.5 + 0.2 * k, p_gain=15.0 + 5.0 * k, kv=0.6 + 0.2 * k)
    env.set_reset_pool("base_payload", **body)
    env.set_reset_pool("action_latency", substeps=np.array([1, 3, 5]))
    env.set_reset_pool("gravity", g=g)
    env.set_reset_pool("servo", rate_limit=np.array([0.1, 0.2, np.inf]), d_gain=0.02 * k)
    env.set_reset_pool("torque_limit", limit=np.array([[3.0, 4.0, 5.0], [6.0, 7.0, 8.0], [np.inf, np.inf, np.inf]]))
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    pool = {kind: n(env.reset_pool(kind)[0]) for kind in ("env_params", "base_payload", "action_latency", "gravity", "servo", "torque_limit")}
    members = privileged_reference(np.zeros((3, 66)), env.privileged_defaults(), base_height=0.0, mu=pool["env_params"][:, 0], p_gain=pool["env_params"][:, 1],
                                   kv=pool["env_params"][:, 2], body_rows=pool["base_payload"], latency=pool["action_latency"], g=pool["gravity"][:, 0:3],
                                   rate_limit=pool["servo"][:, 0], d_gain=pool["servo"][:, 1], torque_limit=pool["torque_limit"][:, :3])[:, 66:]
    groups = dict(env_params=[0, 1, 2], base_payload=[3, 4, 5, 6], action_latency=[7], gravity=[8, 9, 10], servo=[11, 12], torque_limit=[13, 14, 15])

    def member(row):
        return {kind: [j for j in range(3) if np.allclose(row[cols], members[j, cols], rtol=1e-6, atol=0)] for kind, cols in groups.items()}

    obs, priv = env.reset()                 # reset_idx(all): every env has drawn its rows from the pools
    first = _check_row(env, obs, priv)
    assert all(all(m for m in member(first[e]).values()) for e in range(N))
    counts0 = env.reset_row_counts().copy()
    rng = np.random.default_rng(1)
    seen = []
    for t in range(4):
        if t == 2:
            _tilt(env, 3)
        obs, priv, _, done, _ = env.step(torch.from_numpy(rng.uniform(-1, 1, (N, 18)).astype(np.float32)))
        got = _check_row(env, obs, priv)
        assert int(done[3]) == (1 if t == 2 else 0)
        assert np.array_equal(got[[0, 1, 2, 4], :22], first[[0, 1, 2, 4], :22])      # nobody else's rows move
        seen.append(got[3, :22].copy())
        assert all(m for m in member(got[3]).values()), member(got[3])
    assert np.array_equal(seen[0], first[3, :22]) and np.array_equal(seen[1], seen[0]) and np.array_equal(seen[3], seen[2])
    assert (env.reset_row_counts() - counts0).tolist() == [0, 0, 0, 1, 0]
    env.close()


def test_off_is_off_and_on_changes_no_observation():
    """A default config keeps the reference's surface; an env with the switch on returns, in its first 66 columns and in obs_buf, bit for bit
    the observations of an env built from the same config without it (observation noise on: the copy includes noise and clipping)."""
    N = 33
    off, on = _env(N, priv=False, noise=True, seed=5), _env(N, priv=True, noise=True, seed=5)
    assert off.num_privileged_obs == 66 and off.privileged_obs_has_obs_prefix is False and off.get_privileged_observations() is None
    o0, p0 = off.reset()
    o1, p1 = on.reset()
    assert p0 is None and torch.equal(o0, o1) and torch.equal(p1[:, :66], o0)
    plain = make_env(N, seed=5, noise=True)
    assert plain.get_privileged_observations() is None and plain.num_privileged_obs == 66
    assert torch.equal(plain.reset()[0], o0)
    rng = np.random.default_rng(2)
    for t in range(6):
        a = torch.from_numpy(rng.uniform(-1, 1, (N, 18)).astype(np.float32)).to(DEV)
        r0, r1 = off.step(a), on.step(a)
        assert r0[1] is None and off.get_privileged_observations() is None
        assert torch.equal(r0[0], r1[0]) and torch.equal(r1[1][:, :66], r0[0]) and torch.equal(r0[2], r1[2]) and torch.equal(r0[3], r1[3])
    for x, y in zip(off.get_state(), on.get_state()):
        np.testing.assert_array_equal(x, y)
    for e in (off, on, plain):
        e.close()


class _Prefix:
    """An actor-critic as _ppo_reference_losses reads it, with the actor fed the first n columns of the row the critic is fed."""

    def __init__(self, ac, n):
        self.actor, self.critic, self.std = (lambda rows: ac.actor(rows[:, :n])), ac.critic, ac.std


SHAPES = {"A": (66, 89, 18, [54, 42, 30], [54, 42, 30]), "B": (5, 9, 3, [7], [6])}


def _asym(shape, seed=5):
    from nightmare_rl_amd.rl import ActorCritic
    na, nc, A, hid, chid = SHAPES[shape]
    torch.manual_seed(seed)
    ac = ActorCritic(na, nc, A, actor_hidden_dims=hid, critic_hidden_dims=chid, activation="elu", init_noise_std=0.8).to(DEV)
    with torch.no_grad():
        for m in list(ac.actor) + list(ac.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return ac, na, nc, A


def _batch(ref, B, na, nc, A):
    rows = torch.randn(B, nc, device=DEV)
    with torch.no_grad():
        old_mu = ref.actor(rows[:, :na]) + 0.05 * torch.randn(B, A, device=DEV)
        old_sigma = (ref.std * (1 + 0.05 * torch.randn(A, device=DEV))).expand(B, A).contiguous()
        actions = old_mu + old_sigma * torch.randn(B, A, device=DEV)
        old_logp = torch.distributions.Normal(old_mu, old_sigma).log_prob(actions).sum(-1)
        tv = ref.critic(rows).squeeze(-1) + 0.3 * torch.randn(B, device=DEV)
        ret = tv + torch.randn(B, device=DEV)
        adv = torch.randn(B, device=DEV)
    return (rows, actions, tv, adv, ret, old_logp, old_mu, old_sigma)


@pytest.mark.parametrize("B", [151, 7])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_asymmetric_minibatch_matches_torch_autograd_and_adam(shape, B):
    """The body of test_fused_ppo_minibatch_matches_torch_autograd_and_adam (tests/test_gpu_parity.py), tolerances unchanged, with the
    critic fed the wide row and the actor its prefix: shape A 66 -> 54 -> 42 -> 30 -> 18 | 89 -> 54 -> 42 -> 30 -> 1, shape B 5 -> 7 -> 3 |
    9 -> 6 -> 1 (two layers, widths no multiple of 4); B = 151 (9 full tiles and 7 rows) and B = 7. Then the privileged columns of the
    batch are replaced: the actor's and std's gradient entries stay bit-identical, the critic's do not."""
    from nightmare_rl_amd.rl.fused import FusedUpdate
    ac, na, nc, A = _asym(shape)
    ref = copy.deepcopy(ac)
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    assert FusedUpdate.supported(ac, DEV)
    fu = FusedUpdate(ac, opt, DEV, lr=1e-3)
    assert not fu.has_fast_path and fu.n_obs == nc
    hp = dict(clip=0.2, value_coef=1.0, entropy_coef=0.0015, clip_value=True, desired_kl=0.01, adaptive=True, max_grad_norm=1.0)
    lin = lambda net: [q for m in net if isinstance(m, torch.nn.Linear) for q in (m.weight, m.bias)]
    n_actor = sum(p.numel() for p in lin(ac.actor))
    lr = 1e-3
    torch.manual_seed(5)
    for it in range(4):
        mb = _batch(ref, B, na, nc, A)
        loss, surr, vl, kl = _ppo_reference_losses(_Prefix(ref, na), mb)
        klm = float(kl.detach())
        if klm > 0.02:
            lr = max(1e-5, lr / 1.5)
        elif 0.0 < klm < 0.005:
            lr = min(1e-2, lr * 1.5)
        for g in ropt.param_groups:
            g["lr"] = lr
        ropt.zero_grad()
        loss.backward()
        ref_grad = torch.cat([p.grad.reshape(-1) for p in lin(ref.actor) + lin(ref.critic) + [ref.std]])
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0))
        ropt.step()
        # the privileged columns replaced: nothing of the actor's or std's gradient may move, the critic's must
        other = mb[0].clone()
        other[:, na:] = torch.randn(B, nc - na, device=DEV)
        fu.minibatch(other, *mb[1:], hp, phase=1)
        g_other = fu.grad().clone()
        fu.minibatch(*mb, hp, phase=1)
        g = fu.grad().clone()
        err = float((g - ref_grad).abs().max() / ref_grad.abs().max())
        print(f"shape {shape} B {B} step {it}: gradient error {err:.3e} of its max, kl {klm:.4e}")
        assert err < 2e-4, (it, err)
        assert torch.equal(g[:n_actor], g_other[:n_actor]) and torch.equal(g[-A:], g_other[-A:])
        assert not torch.equal(g[n_actor:-A], g_other[n_actor:-A])
        fu.minibatch(*mb, hp, phase=2)
        st = fu.read_state()
        assert abs(st["kl"] - klm) < 1e-5 + 1e-4 * klm, (st["kl"], klm)
        assert abs(st["lr"] - lr) < 1e-9 and abs(st["grad_norm"] - norm) < 1e-4 * norm
        assert abs(st["surrogate_loss_sum"] - float(surr.detach())) < 1e-4 and abs(st["value_loss_sum"] - float(vl.detach())) < 1e-4 * float(vl.detach())
        for (n1, p1), (n2, p2) in zip(ac.named_parameters(), ref.named_parameters()):
            assert n1 == n2
            torch.testing.assert_close(p1, p2, atol=2e-5, rtol=1e-4, msg=lambda m: f"{n1} after step {it}: {m}")
    sd, rsd = opt.state_dict()["state"], ropt.state_dict()["state"]
    for k in sd:
        torch.testing.assert_close(sd[k]["exp_avg"], rsd[k]["exp_avg"], atol=1e-6, rtol=1e-3)
        torch.testing.assert_close(sd[k]["exp_avg_sq"], rsd[k]["exp_avg_sq"], atol=1e-6, rtol=1e-3)
    assert fu.flat.numel() == sum(p.numel() for p in ref.parameters())      # nparam: the real parameters, no padding column among them


def test_collector_feeds_the_critic_the_row_and_the_actor_its_prefix():
    """FusedCollector.act on N = 37 wide rows (three workgroups of the sampling kernel, the last with 5 envs): mu = actor(prefix), value =
    critic(row) (the tolerances of the collector comparison in tests/test_gpu_activations.py), both storage rows bit for bit; again after
    three fused updates (refresh() repacks), where changing the privileged columns leaves mu bit-identical."""
    from nightmare_rl_amd.rl import RolloutStorage
    from nightmare_rl_amd.rl.fused import FusedCollector, FusedUpdate
    N = 37
    ac, na, nc, A = _asym("A")
    with torch.no_grad():
        ac.std.mul_(torch.linspace(0.6, 1.4, A, device=DEV))
    assert FusedCollector.supported(ac, DEV)
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), DEV, lr=1e-3)
    col = FusedCollector(ac, N, DEV, seed=11, update=fu)
    assert col.update is None and col.asymmetric
    st = RolloutStorage(N, 4, [na], [nc], [A], DEV)
    hp = dict(clip=0.2, value_coef=1.0, entropy_coef=0.0015, clip_value=True, desired_kl=0.01, adaptive=True, max_grad_norm=1.0)

    def check(s):
        torch.manual_seed(20 + s)
        rows = torch.randn(N, nc, device=DEV) * 2.0
        st.step = s
        a = col.act(rows, st)
        with torch.no_grad():
            mu, v = ac.actor(rows[:, :na]), ac.critic(rows).squeeze(-1)
        torch.testing.assert_close(st.mu[s], mu, atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(st.values[s].squeeze(-1), v, atol=2e-5, rtol=1e-5)
        assert torch.equal(st.sigma[s], ac.std.detach().expand(N, A)) and a.data_ptr() == st.actions[s].data_ptr()
        assert torch.equal(st.observations[s], rows[:, :na]) and torch.equal(st.privileged_observations[s], rows)
        lp = torch.distributions.Normal(st.mu[s], st.sigma[s]).log_prob(st.actions[s]).sum(-1)
        torch.testing.assert_close(st.actions_log_prob[s].squeeze(-1), lp, atol=2e-4, rtol=1e-5)
        mu_first, v_first = st.mu[s].clone(), st.values[s].clone()
        other = rows.clone()
        other[:, na:] = torch.randn(N, nc - na, device=DEV)
        col.act(other, st)
        assert torch.equal(st.mu[s], mu_first) and not torch.equal(st.values[s], v_first)
        assert torch.equal(st.observations[s], rows[:, :na]) and torch.equal(st.privileged_observations[s], other)

    check(0)
    before = fu.flat.clone()
    torch.manual_seed(9)
    for _ in range(3):
        fu.minibatch(*_batch(ac, 151, na, nc, A), hp)
    col.refresh(1)
    assert not torch.equal(before, fu.flat)
    check(1)
    with pytest.raises(ValueError, match="rows must be"):
        col.act(torch.randn(N, na, device=DEV), st)


def test_runner_trains_an_asymmetric_actor_critic_on_the_kernels():
    """OnPolicyRunner on an env with privileged observations and two randomisation kinds on, N = 64, 8 steps per env, 2 iterations: the
    generic fused update and the per-step collector, 89-wide critic rows in the storage, finite losses, parameters that moved. The same
    networks without the caller's promise about the row's prefix take the torch path."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3ConfigPPO
    from nightmare_rl_amd.rl import PPO, ActorCritic, OnPolicyRunner
    from nightmare_rl_amd.rl.fused import FusedUpdate

    class domain_rand:
        randomize_friction, friction_range = True, (0.5, 1.25)
        randomize_base_mass, added_mass_range = True, (-0.2, 0.4)

    cfg = class_to_dict(NightmareV3ConfigPPO())
    cfg["runner"]["num_steps_per_env"] = 8
    cfg["runner"]["save_interval"] = 1000
    torch.manual_seed(0)
    env = _env(64, seed=1, domain_rand=domain_rand)
    r = OnPolicyRunner(env, cfg, log_dir=None, device=DEV)
    alg = r.alg
    assert alg.fused is not None and alg.fused.asymmetric and isinstance(alg.fused_update, FusedUpdate) and not alg.fused_update.has_fast_path
    assert alg.storage.privileged_observations.shape == (8, 64, 89) and alg.storage.observations.shape == (8, 64, 66)
    assert [m.in_features for m in (alg.actor_critic.actor[0], alg.actor_critic.critic[0])] == [66, 89]
    before = alg.fused_update.flat.clone()
    r.learn(2, init_at_random_ep_len=True)
    assert r.rollout_mode == "per-step launches" and len(r.history) == 2
    assert np.isfinite([h["value_loss"] for h in r.history]).all() and np.isfinite([h["surrogate_loss"] for h in r.history]).all()
    after = alg.fused_update.flat
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    n_actor = sum(p.numel() for p in alg.actor_critic.actor.parameters())
    assert not torch.equal(before[:n_actor], after[:n_actor]) and not torch.equal(before[n_actor:-18], after[n_actor:-18])
    # what the collector filed: the observation is the prefix of the critic's row, whose parameter columns are the drawn ones
    st = alg.storage
    assert torch.equal(st.privileged_observations[..., :66], st.observations)
    mu = st.privileged_observations[..., 66]
    assert float(mu.min()) >= 0.5 and float(mu.max()) < 1.25 and float(mu.std()) > 0.05
    # another env's privileged layout: no promise, no kernels
    ac = ActorCritic(66, 89, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu").to(DEV)
    foreign = PPO(ac, device=DEV)
    foreign.init_storage(64, 8, [66], [89], [18])
    assert foreign.fused is None and foreign.fused_update is None
    env.close()


def test_a_wider_actor_is_refused_with_both_widths():
    from nightmare_rl_amd import _lib
    L = _lib.load()
    a, c = (C.c_int32 * 5)(89, 54, 42, 30, 18), (C.c_int32 * 5)(66, 54, 42, 30, 1)
    h = C.c_void_p()
    assert L.nm_ppo_create_act(a, c, 4, 0, 0, C.byref(h)) != 0 and not h.value
    msg = L.nm_last_error().decode()
    assert "89" in msg and "66" in msg and "nm_ppo_create" in msg
