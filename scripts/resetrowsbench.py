"""Wall time per env step of the K-step launches (step_tape, policy_play, policy_rollout) and of the per-step path (step()), by
torch events around 5 repetitions after a warm-up, three runs each, microseconds per step (K = 80 for `off`, 40 for the other two):
   off     no reset pool (what the parent commit's library computes too: run it with NM_HIP_LIB=<the parent's library>)
   on      all six reset pools installed (1024 rows each, mild values) and 40-step episodes (cfg.env.episode_length_s = 0.64): every env
           times out once per 40 steps
   rows    the same as `on`, but the pools are dropped after the first reset(): every env keeps the rows it drew, all six kinds stay on
           (the same level of the step), and no reset re-draws - the line `on` is to be held against
   off40   the 40-step episodes with no per-env kind on at all
The library that is loaded has no nm_set_reset_rows (the parent's): only `off` is measured.
   python scripts/resetrowsbench.py [N]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd import _lib
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env, gravity_from_draw
from nightmare_rl_amd.rl import ActorCritic, RolloutStorage
from nightmare_rl_amd.rl.fused import FusedUpdate

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K, REPS, RUNS = 80, 5, 3
dev = "cuda:0"
tag = os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH)
has_pools = hasattr(_lib.load(), "nm_set_reset_rows")


def make(mode):
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    if mode != "off":
        cfg.env.episode_length_s = 0.64
    env = NightmareV3Env(cfg, device=dev, seed=0)
    if mode in ("on", "rows"):
        P, rng = 1024, np.random.default_rng(0)
        env.set_reset_pool("env_params", mu=rng.uniform(0.6, 1.2, P), kv=rng.uniform(0.7, 0.9, P))
        env.set_reset_pool("base_payload", dm=rng.uniform(0.0, 0.3, P), r=rng.uniform(-0.02, 0.02, (P, 3)))
        env.set_reset_pool("action_latency", substeps=rng.integers(0, 7, P).astype(np.int32))
        env.set_reset_pool("gravity", g=gravity_from_draw(np.zeros((P, 3)), rng.uniform(0, 0.1, P), rng.uniform(0, 2 * np.pi, P)))
        env.set_reset_pool("servo", rate_limit=rng.uniform(0.2, 0.5, P), d_gain=rng.uniform(0.0, 0.1, P))
        env.set_reset_pool("torque_limit", limit=rng.uniform(3.0, 6.0, (P, 3)))
    env.reset()
    if mode == "rows":
        for kind in ("env_params", "base_payload", "action_latency", "gravity", "servo", "torque_limit"):
            env.set_reset_pool(kind)
    return env


def timed(f):
    res = []
    f()
    for _ in range(RUNS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            f()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / (REPS * K))
    return res


torch.manual_seed(5)
ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu", init_noise_std=0.3).to(dev)
fu = FusedUpdate(ac, torch.optim.Adam(ac.parameters(), lr=1e-3), dev, lr=1e-3)
acts = ((torch.rand(K, N, 18, generator=torch.Generator().manual_seed(0)) * 2 - 1) * 0.12).to(dev).contiguous()
it = torch.tensor([1], dtype=torch.int64, device=dev)
for mode in (("off", "off40", "rows", "on") if has_pools else ("off",)):
    K = 80 if mode == "off" else 40          # nm_rollout takes at most one episode per launch; all paths use the same K per mode
    a = acts[:K].contiguous()
    env = make(mode)
    line = lambda what, r: print(f"{tag}: {what:<14} {mode:<5} N={N} K={K}: us per step " + " ".join(f"{x:.2f}" for x in r), flush=True)
    line("step()", timed(lambda: [env.step(a[i]) for i in range(K)]))
    line("step_tape", timed(lambda: env.step_tape(a)))
    line("policy_play", timed(lambda: env.policy_play(K, fu.flat, seed=7, iter_dev=it)))
    st = RolloutStorage(N, K, [66], [None], [18], dev)
    z = lambda n: torch.zeros(n, device=dev)
    cr, cl, fin = z(N), z(N), z(3)
    line("policy_rollout", timed(lambda: env.policy_rollout(K, fu.flat, 9, it, st, 0.99, cr, cl, fin)))
    if mode == "on":
        print(f"{tag}: re-draws per env in this run: min {int(env.reset_row_counts().min())} max {int(env.reset_row_counts().max())}", flush=True)
    env.close()
