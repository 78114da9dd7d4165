"""Device time of the K-step launches with push perturbations off and on (nm_set_push), by HIP event pairs: the one-launch rollout
(nm_rollout) and the play kernel (nm_play) - microseconds per launch and per env step, `rounds` rounds of 10 launches each.
   python scripts/pushbench.py [N] [K] [rounds] [interval]     (NM_HIP_LIB=<another build> for an A/B on one box: a library without
                                                                 nm_set_push runs the pushes-off lines only)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd import _lib
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
from nightmare_rl_amd.rl import ActorCritic, RolloutStorage
from nightmare_rl_amd.rl.fused import FusedUpdate

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 80
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
interval = int(sys.argv[4]) if len(sys.argv) > 4 else 5
dev = "cuda:0"
torch.manual_seed(0)
ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu", init_noise_std=1.0).to(dev)
fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
z = lambda *s: torch.zeros(*s, device=dev)
it = torch.zeros(1, dtype=torch.int64, device=dev)
has_push = hasattr(_lib.load(), "nm_set_push")


def make(push):
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    env = NightmareV3Env(cfg, device=dev, seed=0)
    env.reset()
    torch.manual_seed(1)
    env.episode_length_buf = torch.randint(0, 1250, (N,), device=dev, dtype=torch.int64)
    if push:
        env.set_push(interval, 0.5)
    return env


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def report(name, ms):
    us = sorted(m * 1e3 for m in ms)
    print(f"{name}: {K} steps x {N} envs per launch: median {us[len(us) // 2]:.1f} us (min {us[0]:.1f}, max {us[-1]:.1f} over {rounds} rounds of 10 launches) "
          f"= {us[len(us) // 2] / K:.2f} us per step = {N * K / us[len(us) // 2]:.2f} M env-steps/s", flush=True)


st = RolloutStorage(N, K, [66], [None], [18], dev)
cur_ret, cur_len, fin = z(N), z(N), z(3)
for push in ((False, True) if has_push else (False,)):
    tag = f"pushes every {interval} steps" if push else "pushes off"
    env = make(push)
    ep_idx = torch.tensor([env._stat_names.index(k[4:]) for k in sorted(env.extras["episode"])], dtype=torch.int32, device=dev)
    ep_acc = z(ep_idx.numel())
    report(f"nm_rollout, {tag}", timed(lambda: env.policy_rollout(K, fu.flat, 1, it, st, 0.99, cur_ret, cur_len, fin, ep=(ep_idx, ep_acc))))
    env.close()
    env = make(push)
    stats = dict(cur_ret=cur_ret, cur_len=cur_len, fin=fin, ret_sum=z(N), ret_cnt=z(N))
    report(f"nm_play (sampled), {tag}", timed(lambda: env.policy_play(K, fu.flat, seed=1, iter_dev=it, stats=stats)))
    env.close()
