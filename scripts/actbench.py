"""Per-activation times of the three kernels that evaluate the networks, at N envs (default 4096):
  * k_mlp_fused on a 66 -> 256 -> 256 -> 18 network (ActorMLP / nm_policy_forward, one launch);
  * one PPO update on the reference networks (66 -> 54 -> 42 -> 30 -> 18 | 1, fast path): the config's epochs x mini-batches of
    nm_ppo_minibatch_rows over an 80-step rollout's rows, permutation included;
  * the 80-step one-launch rollout (nm_rollout_ex: policy + physics + record).
Prints one line per activation (and a JSON list with --json).   python scripts/actbench.py [N] [--json]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd.envs.helpers import class_to_dict  # noqa: E402
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO  # noqa: E402
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env  # noqa: E402
from nightmare_rl_amd.policy import ActorMLP  # noqa: E402
from nightmare_rl_amd.rl import ActorCritic, RolloutStorage  # noqa: E402
from nightmare_rl_amd.rl.fused import FusedCollector, FusedUpdate  # noqa: E402

ACTS = ["elu", "selu", "relu", "lrelu", "tanh", "sigmoid"]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 4096
T = 80
dev = "cuda:0"
alg = class_to_dict(NightmareV3ConfigPPO())["algorithm"]
hp = dict(clip=alg["clip_param"], value_coef=alg["value_loss_coef"], entropy_coef=alg["entropy_coef"], clip_value=alg["use_clipped_value_loss"],
          desired_kl=alg["desired_kl"], adaptive=True, max_grad_norm=alg["max_grad_norm"])
E, MB = alg["num_learning_epochs"], alg["num_mini_batches"]


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


rows = []
for act in ACTS:
    torch.manual_seed(0)
    # k_mlp_fused, 66 -> 256 -> 256 -> 18
    net = ActorMLP([66, 256, 256, 18], activation=act).to(dev)
    x = torch.randn(N, 66, device=dev)
    out = torch.empty(N, 18, device=dev)
    net(x)
    mlp_us = 1e3 * timed(lambda: net._packed.forward(x, out=out), 200)
    # one PPO update on the reference networks (fast path)
    ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation=act, init_noise_std=1.0).to(dev)
    fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
    assert fu.has_fast_path
    R = T * N
    obs = torch.randn(R, 66, device=dev)
    with torch.no_grad():
        mu = ac.actor(obs)
    sig = ac.std.detach().expand(R, 18).contiguous()
    actions = mu + sig * torch.randn(R, 18, device=dev)
    logp = torch.distributions.Normal(mu, sig).log_prob(actions).sum(-1)
    tv, ret, adv = torch.randn(R, device=dev), torch.randn(R, device=dev), torch.randn(R, device=dev)
    mb = R // MB
    perm = fu.permutation(MB * mb, 1, 0)
    count = [0]

    def update():
        count[0] += 1
        fu.permutation(MB * mb, 1, count[0], out=perm)
        for _ in range(E):
            for i in range(MB):
                fu.minibatch(obs, actions, tv, adv, ret, logp, mu, sig, hp, rows=perm[i * mb:(i + 1) * mb])

    upd_ms = timed(update, 5, warm=1)
    # the 80-step one-launch rollout
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    env = NightmareV3Env(cfg, device=dev, seed=0)
    env.reset()
    env.episode_length_buf = torch.randint(0, 1250, (N,), device=dev, dtype=torch.int64)
    col = FusedCollector(ac, N, dev, seed=1, update=fu)
    assert col.can_rollout(env)
    st = RolloutStorage(N, T, [66], [None], [18], dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    cur_ret, cur_len, fin = z(N), z(N), z(3)
    roll_ms = timed(lambda: col.rollout(env, st, T, 0.99, cur_ret, cur_len, fin), 5, warm=2)
    env.close()
    r = dict(activation=act, N=N, mlp_fused_us=round(mlp_us, 2), ppo_update_ms=round(upd_ms, 3), minibatches=E * MB,
             rollout_ms=round(roll_ms, 3), rollout_Msteps_s=round(N * T / roll_ms / 1e3, 2))
    rows.append(r)
    print(f"{act:8s} k_mlp_fused {mlp_us:8.2f} us | PPO update ({E * MB} mini-batches) {upd_ms:7.3f} ms | {T}-step rollout {roll_ms:7.3f} ms "
          f"= {r['rollout_Msteps_s']:.2f} M env-steps/s", flush=True)
if "--json" in sys.argv:
    print(json.dumps(rows))
