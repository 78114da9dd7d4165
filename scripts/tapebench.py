"""Device time per env step of stepping from known actions, by HIP event pairs, at N envs (default 4096) after 20 settling steps:
  (a) K = 80 x env.step(actions[t])            - one nm_step launch per row, the per-step path
  (b) one env.step_tape(actions) of the same K rows - nm_step_tape, one launch
from the same start state (saved after settling and restored before every leg), and the scripted gait engine driving the env
(scripts/custom_play.py): its per-step loop (gait tick, rate limit, action mapping, step) against the two-launch form (EngineNode.tape +
step_tape) over K steps. Medians over `rounds`; one JSON line.
   python scripts/tapebench.py [N] [K] [rounds]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nightmare_rl_amd import nikengine as nk
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 80
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
SETTLE = 20
dev = "cuda:0"

cfg = NightmareV3Config()
cfg.env.num_envs = N
env = NightmareV3Env(cfg, device=dev, seed=0)
env.reset()
g = torch.Generator(device="cpu").manual_seed(1)
env.episode_length_buf = torch.randint(0, int(env.max_episode_length) - 1, (N,), generator=g).to(dev)
settle = (torch.rand(SETTLE, N, 18, generator=g) * 2 - 1).to(dev)
actions = (torch.rand(K, N, 18, generator=g) * 2 - 1).to(dev).contiguous()
for t in range(SETTLE):
    env.step(settle[t])
torch.cuda.synchronize()
saved = (env.get_state(), env.get_buffers(), env.get_feet_state(), env.episode_length_buf.clone())


def restore():
    (qpos, qvel, qw), b, (air, last, filt), ep = saved
    env.set_state(qpos, qvel, qw)
    env.set_buffers(dof_pos=b["dof_pos"], dof_vel=b["dof_vel"], actions=b["actions"], commands=b["commands"], episode_sums=b["episode_sums"])
    env.set_feet_state(air, last, filt)
    env.episode_length_buf = ep.clone()
    torch.cuda.synchronize()


def timed(fn):
    """milliseconds of fn() between two events on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def per_step():
    for t in range(K):
        env.step(actions[t])


def median(x):
    return sorted(x)[len(x) // 2]


# ---- (a) / (b): the same K action rows from the same start state
legs = {"step_loop": per_step, "step_tape": lambda: env.step_tape(actions)}
ms = {k: [] for k in legs}
for r in range(rounds + 1):              # round 0 warms up
    for name, fn in legs.items():
        restore()
        t = timed(fn)
        if r:
            ms[name].append(t)
a_us, b_us = (median(ms[k]) * 1e3 / K for k in ("step_loop", "step_tape"))

# ---- custom_play: the per-step loop against the two-launch form
nk.config.ENGINE_FPS = 1.0 / env.dt
lin = torch.full((N,), 0.05, device=dev, dtype=torch.float64)
ang = torch.zeros(N, device=dev, dtype=torch.float64)
engs = {"custom_play_loop": nk.EngineNode(N, device=dev), "custom_play_two_launch": nk.EngineNode(N, device=dev)}
targets = torch.zeros(N, 18, device=dev)
servo = env.joint_target_servo(0.08)
tick = {k: 0 for k in engs}


def play_loop():
    eng = engs["custom_play_loop"]
    for i in range(K):
        goal = eng.update(lin, ang, "awake", "walk", time_s=(tick["custom_play_loop"] + i) * env.dt)
        targets.add_(torch.clamp(goal - targets, -0.08, 0.08))
        env.step(env.actions_from_joint_targets(targets))
    tick["custom_play_loop"] += K


def play_two():
    tape = engs["custom_play_two_launch"].tape(lin, ang, "awake", "walk", steps=K, tick0=tick["custom_play_two_launch"], dt=env.dt, servo=servo)
    env.step_tape(tape)
    tick["custom_play_two_launch"] += K


cp = {"custom_play_loop": [], "custom_play_two_launch": []}
for r in range(rounds + 1):
    for name, fn in (("custom_play_loop", play_loop), ("custom_play_two_launch", play_two)):
        restore()
        t = timed(fn)
        if r:
            cp[name].append(t)
c_us, d_us = (median(cp[k]) * 1e3 / K for k in ("custom_play_loop", "custom_play_two_launch"))
print(json.dumps({"bench": "tapebench", "num_envs": N, "steps": K, "rounds": rounds, "settling_steps": SETTLE,
                  "step_loop_us_per_step": round(a_us, 2), "step_tape_us_per_step": round(b_us, 2), "step_loop_over_step_tape": round(a_us / b_us, 3),
                  "step_loop_us_rounds": [round(m * 1e3 / K, 2) for m in ms["step_loop"]],
                  "step_tape_us_rounds": [round(m * 1e3 / K, 2) for m in ms["step_tape"]],
                  "custom_play_loop_us_per_step": round(c_us, 2), "custom_play_two_launch_us_per_step": round(d_us, 2),
                  "custom_play_loop_over_two_launch": round(c_us / d_us, 3),
                  "env_steps_per_s_step_loop": round(N / a_us * 1e6), "env_steps_per_s_step_tape": round(N / b_us * 1e6)}))
env.close()
