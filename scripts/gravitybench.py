"""Device time of the step kernel at every level of the per-env rows with DEFAULT rows (so every level computes what level 0 computes and
only the level's own loads and instructions differ), by HIP events (env.profile), in both contact regimes of scripts/quickbench.py (action
scale 1.0 flailing, 0.12 standing; microseconds per launch, three runs of 200 launches each):
   level 0  nothing set                       level 1  default friction / gain rows
   level 2  default body rows                 level 3  latency on with zero delays
   level 4  gravity on with (0, 0, -9.81) twice in every env
The cost of level 4 is the line of level 4 against the line of level 3.
   python scripts/gravitybench.py [N]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd import _lib
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
dev = "cuda:0"
tag = os.path.basename(_lib.LIB_PATH)


def make(level):
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    env = NightmareV3Env(cfg, device=dev, seed=0)
    env.reset()
    if level == 1:
        mu, pg, kv = env._envp_default
        env.set_env_params(mu=mu, p_gain=pg, kv=kv)
    elif level == 2:
        env.set_base_payload(0.0)
    elif level == 3:
        env.set_action_latency(0)
    elif level == 4:
        env.set_gravity([0.0, 0.0, -9.81])
    return env


acts = (torch.rand(16, N, 18, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
for scale in (1.0, 0.12):
    for level in range(5):
        env = make(level)
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
        print(f"{tag}: step kernel, level {level} with default rows, action scale {scale}, N={N}: avg us " + " ".join(f"{r:.2f}" for r in res), flush=True)
        env.close()
