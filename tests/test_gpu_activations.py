"""Every hidden-layer activation of rsl_rl v1.0.2's get_activation (reference envs/nightmare_v3_config.py:109) on the hand-written kernels:
the MFMA policy forward (nm_policy_*), the fused PPO mini-batch (nm_ppo_*: the reference shape's register-resident fast path and the generic
kernel), the collection kernels (nm_ppo_act, the rollout's wave code) and the one-launch rollout, against torch - and the runner end to end.

Tolerances are ELU's: the activations are evaluated with the hardware exponential and reciprocal (nightmare_rl_amd/csrc/nm_act.h: absolute
error < 3e-7 for every sequence, tanh and sigmoid included), well inside the 2e-5 the f32 GEMM chains in another summation order need."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import _ppo_reference_losses, make_env
from test_gpu_rollout import _record, _storage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = ["elu", "selu", "relu", "lrelu", "tanh", "sigmoid"]
REF_HID = [54, 42, 30]


def _ac(act, hid=REF_HID, chid=None, std=0.8, seed=5):
    from nightmare_rl_amd.rl import ActorCritic
    torch.manual_seed(seed)
    ac = ActorCritic(66, 66, 18, actor_hidden_dims=hid, critic_hidden_dims=chid or hid, activation=act, init_noise_std=std).to(DEV)
    with torch.no_grad():      # biases away from zero, distinct std per action: nothing in the packing may hide behind a default
        for m in list(ac.actor) + list(ac.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
        ac.std.mul_(torch.linspace(0.6, 1.4, 18, device=DEV))
    return ac


@pytest.mark.parametrize("act", ACTS)
def test_policy_forward_matches_torch(act):
    """k_mlp_fused<act> (last layer on the previous layer's registers; odd K) and the per-layer k_linear_mfma fallback (> 256 wide),
    one layer (no activation at all), against ActorMLP.torch_forward with the same activation."""
    from nightmare_rl_amd.policy import ActorMLP
    torch.manual_seed(0)
    for dims in ([66, 256, 256, 18], [66, 54, 42, 30, 18], [66, 512, 128, 18], [66, 18]):
        net = ActorMLP(dims, activation=act).cuda()
        x = torch.randn(4096 if dims[1] != 18 else 1000, 66, device=DEV)
        torch.testing.assert_close(net(x), net.torch_forward(x), atol=2e-5, rtol=1e-5, msg=lambda m: f"{act} {dims}: {m}")


@pytest.mark.parametrize("shape", ["reference-fast", "other"])
@pytest.mark.parametrize("act", ACTS)
def test_fused_ppo_minibatch_matches_torch_autograd_and_adam(act, shape):
    """nm_ppo_minibatch with hidden activation `act` (backward from the post-activation values: nmact::dfy) against torch autograd +
    torch.optim.Adam over 4 mini-batches: gradient, KL, learning rate, gradient norm, losses, parameters. The reference shape on
    k_ppo_fwdbwd_split<act>, another shape on the generic k_ppo_fwdbwd with the activation as an argument."""
    from nightmare_rl_amd.rl.fused import FusedUpdate
    hid, chid = ([40, 24, 20], [20, 24, 40]) if shape == "other" else (REF_HID, REF_HID)
    ac = _ac(act, hid, chid)
    torch.manual_seed(5)
    B = 4096 * 5 + 7
    ref = copy.deepcopy(ac)
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    assert FusedUpdate.supported(ac, DEV)
    fu = FusedUpdate(ac, opt, DEV, lr=1e-3)
    assert fu.has_fast_path == (shape == "reference-fast")
    hp = dict(clip=0.2, value_coef=1.0, entropy_coef=0.0015, clip_value=True, desired_kl=0.01, adaptive=True, max_grad_norm=1.0)
    lr = 1e-3
    for it in range(4):
        obs = torch.randn(B, 66, device=DEV)
        with torch.no_grad():
            old_mu = ref.actor(obs) + 0.05 * torch.randn(B, 18, device=DEV)
            old_sigma = (ref.std * (1 + 0.05 * torch.randn(18, device=DEV))).expand(B, 18).contiguous()
            actions = old_mu + old_sigma * torch.randn(B, 18, device=DEV)
            old_logp = torch.distributions.Normal(old_mu, old_sigma).log_prob(actions).sum(-1)
            tv = ref.critic(obs).squeeze(-1) + 0.3 * torch.randn(B, device=DEV)
            ret = tv + torch.randn(B, device=DEV)
            adv = torch.randn(B, device=DEV)
        mb = (obs, actions, tv, adv, ret, old_logp, old_mu, old_sigma)
        loss, surr, vl, kl = _ppo_reference_losses(ref, mb)
        klm = float(kl.detach())
        if klm > 0.02:
            lr = max(1e-5, lr / 1.5)
        elif 0.0 < klm < 0.005:
            lr = min(1e-2, lr * 1.5)
        for g in ropt.param_groups:
            g["lr"] = lr
        ropt.zero_grad()
        loss.backward()
        lin = lambda net: [q for m in net if isinstance(m, torch.nn.Linear) for q in (m.weight, m.bias)]
        ref_grad = torch.cat([p.grad.reshape(-1) for p in lin(ref.actor) + lin(ref.critic) + [ref.std]])
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0))
        ropt.step()
        fu.minibatch(*mb, hp, phase=1)
        err = float((fu.grad() - ref_grad).abs().max() / ref_grad.abs().max())
        assert err < 2e-4, (act, it, err)
        fu.minibatch(*mb, hp, phase=2)
        st = fu.read_state()
        assert abs(st["kl"] - klm) < 1e-5 + 1e-4 * klm, (st["kl"], klm)
        assert abs(st["lr"] - lr) < 1e-9 and abs(st["grad_norm"] - norm) < 1e-4 * norm
        assert abs(st["surrogate_loss_sum"] - float(surr)) < 1e-4 and abs(st["value_loss_sum"] - float(vl)) < 1e-4 * float(vl)
        for (n1, p1), (n2, p2) in zip(ac.named_parameters(), ref.named_parameters()):
            assert n1 == n2
            torch.testing.assert_close(p1, p2, atol=2e-5, rtol=1e-4, msg=lambda m: f"{act}: {n1} after step {it}: {m}")


@pytest.mark.parametrize("act", ACTS)
def test_collection_kernels_match_torch_and_share_the_noise(act):
    """nm_ppo_act (k_ppo_act_fast<act>, 16x16x4 tiles) and the rollout's wave code (env.policy_act -> nm_rollout_act_ex, 4x4x1 blocks) for
    N = 1001 (half a wave empty): means and values against torch, the same standard-normal draw on both paths."""
    from nightmare_rl_amd import _lib
    from nightmare_rl_amd.rl.fused import FusedUpdate
    N = 1001
    ac = _ac(act)
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), DEV, lr=1e-3)
    assert fu.has_fast_path
    env = make_env(N)
    st, st2 = _storage(N, 3), _storage(N, 3)
    obs = torch.randn(N, 66, device=DEV) * 2.0
    it = torch.tensor([7], dtype=torch.int64, device=DEV)
    env.policy_act(fu.flat, obs, 1234, it, 2, st, activation=act)
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.nm_ppo_act(fu._h, fu.flat.data_ptr(), obs.data_ptr(), N, 1234, it.data_ptr(), 2, st2.actions[2].data_ptr(), st2.actions_log_prob[2].data_ptr(),
                            st2.values[2].data_ptr(), st2.mu[2].data_ptr(), st2.sigma[2].data_ptr(), st2.observations[2].data_ptr(), stream))
    with torch.no_grad():
        mu, v = ac.actor(obs), ac.critic(obs).squeeze(-1)
    for s in (st, st2):
        torch.testing.assert_close(s.mu[2], mu, atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(s.values[2].squeeze(-1), v, atol=2e-5, rtol=1e-5)
        assert torch.equal(s.sigma[2], ac.std.detach().expand(N, 18)) and torch.equal(s.observations[2], obs)
        lp = torch.distributions.Normal(s.mu[2], s.sigma[2]).log_prob(s.actions[2]).sum(-1)
        torch.testing.assert_close(s.actions_log_prob[2].squeeze(-1), lp, atol=2e-4, rtol=1e-5)
    z, z2 = (st.actions[2] - st.mu[2]) / st.sigma[2], (st2.actions[2] - st2.mu[2]) / st2.sigma[2]
    torch.testing.assert_close(z, z2, atol=2e-5, rtol=0)
    assert abs(float(z.mean())) < 0.03 and abs(float(z.std()) - 1.0) < 0.03
    env.close()


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_one_launch_rollout_equals_the_step_by_step_path_bit_for_bit(act):
    """nm_rollout_ex(K = 40, act) against 40 x [nm_rollout_act_ex, nm_step, nm_ppo_record] at N = 63 (odd: half a wave empty). sigmoid is
    the activation with act(0) != 0, i.e. the one that would expose a padding neuron that is not multiplied by a zero weight."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, T, gamma = 63, 40, 0.99
    ac = _ac(act)
    from nightmare_rl_amd.rl.fused import FusedUpdate
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), DEV, lr=1e-3)
    envs = [make_env(N, seed=11), make_env(N, seed=11)]
    for e in envs:
        e.reset()
        torch.manual_seed(3)
        e.episode_length_buf = torch.randint(0, 1250, (N,), device=DEV, dtype=torch.int64)
        e.episode_length_buf[:8] = 1249 - torch.arange(8, device=DEV) * 5      # time-outs inside the rollout
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    ep_idx = torch.tensor([envs[0]._stat_names.index(k[4:]) for k in sorted(envs[0].extras["episode"])], dtype=torch.int32, device=DEV)
    book = [dict(cur_ret=torch.zeros(N, device=DEV), cur_len=torch.zeros(N, device=DEV), fin=torch.zeros(3, device=DEV), ep_acc=torch.zeros(ep_idx.numel(), device=DEV))
            for _ in envs]
    sa, sb = _storage(N, T), _storage(N, T)
    ea, eb, ba, bb = envs[0], envs[1], book[0], book[1]
    lv = torch.full((N,), float("nan"), device=DEV)
    oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]), last_values=lv, activation=act)
    o = eb.get_observations()
    for s in range(T):
        a = eb.policy_act(fu.flat, o, 99, it, s, sb, activation=act)
        o, _, _, _, _ = eb.step(a)
        _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
    torch.cuda.synchronize()
    for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(sa, name), getattr(sb, name)), (act, name, (getattr(sa, name).float() - getattr(sb, name).float()).abs().max())
    assert torch.equal(oa, o) and torch.equal(ea.rew_buf, eb.rew_buf) and torch.equal(ea.reset_buf, eb.reset_buf)
    assert int(sb.dones.sum()) >= 8
    tmp = _storage(N, 1)
    eb.policy_act(fu.flat, o, 99, it, 0, tmp, activation=act)
    assert torch.equal(lv, tmp.values[0].view(-1))
    with torch.no_grad():
        torch.testing.assert_close(lv, ac.evaluate(o).view(-1), atol=3e-5, rtol=1e-5)
    for x, y in zip(ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
    for e in envs:
        e.close()


def test_runner_trains_a_tanh_network_on_the_fused_kernels(tmp_path):
    """OnPolicyRunner (reference train.py:54) with cfg policy.activation = "tanh": the update on the fast path, the rollout as one launch,
    three iterations with finite losses; the checkpoint loads back, and scripts/play.py's loader (told the activation, which a checkpoint
    does not record) reproduces the actor on the MFMA path."""
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3ConfigPPO
    from nightmare_rl_amd.rl import OnPolicyRunner
    cfg = class_to_dict(NightmareV3ConfigPPO())
    cfg["policy"]["activation"] = "tanh"
    cfg["runner"]["save_interval"] = 1000
    torch.manual_seed(0)
    env = make_env(512, seed=1)
    r = OnPolicyRunner(env, cfg, log_dir=str(tmp_path), device=DEV)
    assert r.alg.actor_critic.activation_name == "tanh"
    assert r.alg.fused_update is not None and r.alg.fused_update.has_fast_path
    assert r.alg.fused is not None and r.alg.fused.can_rollout(env)
    r.learn(3, init_at_random_ep_len=True)
    assert r.rollout_mode.startswith("one launch")
    assert np.isfinite([h["value_loss"] for h in r.history]).all() and np.isfinite([h["surrogate_loss"] for h in r.history]).all()
    path = str(tmp_path / "model_3.pt")
    assert os.path.exists(path)
    r2 = OnPolicyRunner(make_env(512, seed=2), cfg, log_dir=None, device=DEV)
    r2.load(path)
    for (n1, p1), (n2, p2) in zip(r.alg.actor_critic.state_dict().items(), r2.alg.actor_critic.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    from play import actor_from_checkpoint
    net, std = actor_from_checkpoint(path, torch.device("cuda", 0), "tanh")
    assert net.activation == "tanh"
    x = torch.randn(1000, 66, device=DEV)
    with torch.no_grad():
        torch.testing.assert_close(net(x), r2.alg.actor_critic.act_inference(x), atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(std, torch.load(path, map_location="cpu")["model_state_dict"]["std"].cuda())
    r2.env.close()
    env.close()
