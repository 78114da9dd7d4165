"""What privileged critic observations (cfg.env.privileged_obs) cost and what the asymmetric PPO path gains, at N envs (default 4096):
   A  k_priv_obs alone: microseconds per launch of nm_privileged_obs by HIP events around 200 back-to-back launches (three runs), with no
      per-env rows (the default values) and with rows set ("every kind set": friction / gain rows and a base wrench - the block is then
      allocated, and the kernel reads every region of it whichever kinds are on)
   B  env-steps/s of step() under random actions with the switch off and on, alternating (three runs of 300 steps each, a host clock
      around work that ends in a device synchronise)
   C  one PPO iteration (N x 80 steps, the config's 5 epochs x 4 mini-batches), seconds and env-steps/s, the median of the last three of
      six iterations, for
        asymmetric, kernels   privileged observations on, the generic fused update + per-step collector (the new path)
        asymmetric, torch     the same env and networks with critic_has_obs_prefix = False: the torch path (what this configuration ran on
                              before the kernels took asymmetric input)
        symmetric             privileged observations off: the register-resident update and the one-launch rollout
   python scripts/privobsbench.py [N]"""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd import _lib
from nightmare_rl_amd.envs.helpers import class_to_dict
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
from nightmare_rl_amd.rl import OnPolicyRunner

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
dev = "cuda:0"
tag = os.path.basename(_lib.LIB_PATH)


class PrivConfig(NightmareV3Config):
    class env(NightmareV3Config.env):
        privileged_obs = True


def make(priv, seed=0):
    cfg = (PrivConfig if priv else NightmareV3Config)()
    cfg.env.num_envs = N
    return NightmareV3Env(cfg, device=dev, seed=seed)


# ---- A: the gather kernel alone
for rows in ("no rows", "every kind set"):
    env = make(True)
    if rows != "no rows":
        env.set_env_params(mu=torch.linspace(0.5, 1.25, N), p_gain=20.0, kv=0.8)
        env.set_base_wrench([1.0, 0.0, 0.0], [0.0, 0.1, 0.0])
    env.reset()
    L, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    launch = lambda: _lib.check(L.nm_privileged_obs(env._h, env.obs_buf.data_ptr(), env.privileged_obs_buf.data_ptr(), stream))
    for _ in range(50):
        launch()
    res = []
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1) / 200 * 1e3)
    print(f"{tag}: A k_priv_obs, {rows}, N={N}: us per launch (200 back to back) " + " ".join(f"{r:.2f}" for r in res), flush=True)
    env.close()

# ---- B: step() with the switch off and on
acts = (torch.rand(16, N, 18, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
envs = {"off": make(False), "on": make(True)}
for e in envs.values():
    e.reset()
    for i in range(300):
        e.step(acts[i % 16])
rate = {"off": [], "on": []}
for rep in range(3):
    for name, e in envs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(300):
            e.step(acts[i % 16])
        torch.cuda.synchronize()
        rate[name].append(300 * N / (time.perf_counter() - t0))
for name in rate:
    print(f"{tag}: B step(), privileged_obs {name}, N={N}: env-steps/s " + " ".join(f"{r:.4e}" for r in rate[name]), flush=True)
for e in envs.values():
    e.close()

# ---- C: one PPO iteration end to end
for name, priv, promise in (("asymmetric, kernels", True, True), ("asymmetric, torch", True, False), ("symmetric", False, True)):
    torch.manual_seed(0)
    env = make(priv, seed=1)
    if not promise:
        env.privileged_obs_has_obs_prefix = False      # the runner then makes no promise about the row: PPO keeps its torch path
    cfg = class_to_dict(NightmareV3ConfigPPO())
    cfg["runner"]["save_interval"] = 10 ** 9
    r = OnPolicyRunner(env, cfg, log_dir=None, device=dev)
    r.learn(6, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    t = [h["collection_time"] + h["learn_time"] for h in r.history[-3:]]
    c = [h["collection_time"] for h in r.history[-3:]]
    T = cfg["runner"]["num_steps_per_env"]
    kind = "fused update" + (" (fast path)" if r.alg.fused_update.has_fast_path else " (generic)") if r.alg.fused_update is not None else "torch update"
    print(f"{tag}: C PPO iteration, {name}, N={N} x {T}: {kind}, rollout {r.rollout_mode}: median {statistics.median(t) * 1e3:.2f} ms "
          f"(collection {statistics.median(c) * 1e3:.2f} ms), {N * T / statistics.median(t):.4e} env-steps/s; last three " + " ".join(f"{x * 1e3:.2f}" for x in t), flush=True)
    env.close()
