"""Device time of the stepping paths with randomised reset states off and on (nm_set_reset_noise), by HIP event pairs: the per-step path
(nm_step, with the extra k_reset_noise launch behind every step while the feature is on), the one-launch rollout (nm_rollout) and the
play kernel (nm_play) - microseconds per launch and per env step, `rounds` rounds of 10 launches each.
   python scripts/resetnoisebench.py [N] [K] [rounds] [episode_steps]
`episode_steps` (default 40) shortens the episodes so that resets - the only steps on which the feature does anything - are frequent: with
K = 80 every env resets twice per K-step launch. NM_HIP_LIB=<another build> for an A/B on one box: a library without nm_set_reset_noise runs
the feature-off lines only."""
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
ep_steps = int(sys.argv[4]) if len(sys.argv) > 4 else 40
dev = "cuda:0"
RANGES = ((0.0, 0.02), (-0.1, 0.1), (-0.3, 0.3), (-0.3, 0.3), (-0.5, 0.5))
torch.manual_seed(0)
ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu", init_noise_std=1.0).to(dev)
fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
z = lambda *s: torch.zeros(*s, device=dev)
it = torch.zeros(1, dtype=torch.int64, device=dev)
has_feature = hasattr(_lib.load(), "nm_set_reset_noise")


def make(on):
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    cfg.env.episode_length_s = ep_steps * 0.008 * cfg.control.decimation
    env = NightmareV3Env(cfg, device=dev, seed=0)
    if on:
        env.set_reset_noise(RANGES)
    env.reset()
    torch.manual_seed(1)
    env.episode_length_buf = torch.randint(0, int(env.max_episode_length), (N,), device=dev, dtype=torch.int64)
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


def report(name, ms, steps):
    us = sorted(m * 1e3 for m in ms)
    print(f"{name}: {steps} steps x {N} envs per call: median {us[len(us) // 2]:.1f} us (min {us[0]:.1f}, max {us[-1]:.1f} over {rounds} rounds of 10 calls) "
          f"= {us[len(us) // 2] / steps:.2f} us per step = {N * steps / us[len(us) // 2]:.2f} M env-steps/s", flush=True)


Kr = min(K, ep_steps)        # nm_rollout takes at most one episode's steps per launch
st = RolloutStorage(N, Kr, [66], [None], [18], dev)
cur_ret, cur_len, fin = z(N), z(N), z(3)
acts = torch.rand(N, 18, device=dev) * 2 - 1
for on in ((False, True) if has_feature else (False,)):
    tag = "reset noise on" if on else "reset noise off"
    env = make(on)

    def steps20():
        for _ in range(20):
            env.step(acts)
    report(f"nm_step x 20, {tag}", timed(steps20), 20)
    env.close()
    env = make(on)
    ep_idx = torch.tensor([env._stat_names.index(k[4:]) for k in sorted(env.extras["episode"])], dtype=torch.int32, device=dev)
    ep_acc = z(ep_idx.numel())
    report(f"nm_rollout, {tag}", timed(lambda: env.policy_rollout(Kr, fu.flat, 1, it, st, 0.99, cur_ret, cur_len, fin, ep=(ep_idx, ep_acc))), Kr)
    env.close()
    env = make(on)
    stats = dict(cur_ret=cur_ret, cur_len=cur_len, fin=fin, ret_sum=z(N), ret_cnt=z(N))
    report(f"nm_play (sampled), {tag}", timed(lambda: env.policy_play(K, fu.flat, seed=1, iter_dev=it, stats=stats)), K)
    env.close()
