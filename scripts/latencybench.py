"""Device time with per-env actuation latency off and on (draw_action_latency on [0, 6] substeps: level 3 of the step against level 0),
by HIP events: the step kernel in both contact regimes of scripts/quickbench.py (action scale 1.0 flailing, 0.12 standing;
microseconds per launch) and the K-step launches (nm_rollout, nm_play, nm_step_tape; microseconds per launch).
   python scripts/latencybench.py [N] [K] [rounds]     (NM_HIP_LIB=<another build> for an A/B on one box: a library without
                                                         nm_set_action_latency runs the off lines only)"""
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
dev = "cuda:0"
has = hasattr(_lib.load(), "nm_set_action_latency")
tag = os.path.basename(_lib.LIB_PATH)


def make(on):
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    env = NightmareV3Env(cfg, device=dev, seed=0)
    env.reset()
    if on:      # the whole admissible range: neighbours in a wave mostly switch their command at different substeps
        env.draw_action_latency(0, 6)
    return env


acts = (torch.rand(16, N, 18, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
for on in ((False, True) if has else (False,)):
    for scale in (1.0, 0.12):
        env = make(on)
        a = acts * scale
        for i in range(300):
            env.step(a[i % 16])
        res = []
        for rep in range(3):
            env.profile(True)
            for i in range(200):
                env.step(a[i % 16])
            ms, n = env.profile(False)
            res.append(ms / n * 1e3)
        print(f"{tag}: step kernel, latency {'on' if on else 'off'}, action scale {scale}, N={N}: avg us " + " ".join(f"{r:.2f}" for r in res), flush=True)
        env.close()

torch.manual_seed(0)
ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu", init_noise_std=1.0).to(dev)
fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
z = lambda *s: torch.zeros(*s, device=dev)
it = torch.zeros(1, dtype=torch.int64, device=dev)


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
    print(f"{tag}: {name}: {K} steps x {N} envs per launch: median {us[len(us) // 2]:.1f} us (min {us[0]:.1f}, max {us[-1]:.1f} over {rounds} rounds of 10 launches) "
          f"= {us[len(us) // 2] / K:.2f} us per step", flush=True)


st = RolloutStorage(N, K, [66], [None], [18], dev)
cur_ret, cur_len, fin = z(N), z(N), z(3)
for on in ((False, True) if has else (False,)):
    what = f"latency {'on' if on else 'off'}"
    env = make(on)
    torch.manual_seed(1)
    env.episode_length_buf = torch.randint(0, 1250, (N,), device=dev, dtype=torch.int64)
    ep_idx = torch.tensor([env._stat_names.index(k[4:]) for k in sorted(env.extras["episode"])], dtype=torch.int32, device=dev)
    ep_acc = z(ep_idx.numel())
    report(f"nm_rollout, {what}", timed(lambda: env.policy_rollout(K, fu.flat, 1, it, st, 0.99, cur_ret, cur_len, fin, ep=(ep_idx, ep_acc))))
    env.close()
    env = make(on)
    env.episode_length_buf = torch.randint(0, 1250, (N,), device=dev, dtype=torch.int64)
    stats = dict(cur_ret=cur_ret, cur_len=cur_len, fin=fin, ret_sum=z(N), ret_cnt=z(N))
    report(f"nm_play (sampled), {what}", timed(lambda: env.policy_play(K, fu.flat, seed=1, iter_dev=it, stats=stats)))
    env.close()
    env = make(on)
    env.episode_length_buf = torch.randint(0, 1250, (N,), device=dev, dtype=torch.int64)
    tape = (torch.rand(K, N, 18, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev).contiguous()
    report(f"nm_step_tape, {what}", timed(lambda: env.step_tape(tape)))
    env.close()
