"""Device time of the step kernel at levels 0, 6 and 7 of the per-env rows with DEFAULT rows (so every level computes what level 0 computes
and only the level's own loads and instructions differ), by HIP events (env.profile), in both contact regimes of scripts/quickbench.py
(action scale 1.0 flailing, 0.12 standing; microseconds per launch, three runs of 200 launches each):
   level 0  nothing set
   level 6  the servo torque limit on with (inf, inf, inf) in every env: no limit
   level 7  the external wrench on the base on with zero rows in every env: no wrench
   level 7* the same with F = (3, -2, 4) N and tau = (0.3, -0.2, 0.25) N m on every env: a different trajectory
The cost of level 7 is the line of level 7 against the line of level 6.
   python scripts/wrenchbench.py [N]"""
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
    if level == "6":
        env.set_torque_limit(float("inf"))
    elif level == "7":
        env.set_base_wrench([0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    elif level == "7*":
        env.set_base_wrench([3.0, -2.0, 4.0], [0.3, -0.2, 0.25])
    return env


acts = (torch.rand(16, N, 18, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
for scale in (1.0, 0.12):
    for level in ("0", "6", "7", "7*"):
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
        print(f"{tag}: step kernel, level {level}, action scale {scale}, N={N}: avg us " + " ".join(f"{r:.2f}" for r in res), flush=True)
        env.close()
