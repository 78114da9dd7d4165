#!/usr/bin/env python
"""play.py - headless analogue of the reference's play.py (reference play.py:60-72 loads `model_<it>.pt['model_state_dict']` into
an ActorCritic, :118-132 runs `nn.act(obs)` -> scale/clip -> PD servo command -> mj_step in a viewer loop).

Here: the checkpoint's actor runs on the matrix cores (nm_policy_* handle), the env on the step kernel, any number of robots at
once, no viewer. Like upstream the actions are SAMPLED (`nn.act`, not `act_inference`) unless --deterministic.

  python scripts/play.py [checkpoint.pt | --log-root logs/nightmare_v3] [-e 64] [--steps 1300] [--decimation 2] [--cmd 0.3 0.0 0.2]
                         [--activation elu] [--one-launch [--launch-steps K]] [--record-states DIR]
                         [--push-interval-s S [--push-vel V]] [--friction-range LO HI] [--gain-range LO HI]

--one-launch runs the same loop inside the env's own wavefronts (NightmareV3Env.policy_play -> nm_play: policy and step, K steps per
launch, no host round trip per step) and prints the same summary from the device bookkeeping; the actions are then drawn by the
rollout's counter generator, not torch's. --record-states DIR writes upstream's state log of env 0 (envs/nightmare_v3_env.py:261-272),
the files open_custom_play.py:50-66 replays. With --one-launch, --cmd holds (VX, YAW) through set_fixed_commands (VY must be 0: the
env never commands a lateral velocity, :330).

A checkpoint does not record the hidden activation of its networks (rsl_rl saves the state_dict only): --activation names it, by default
the training config's (NightmareV3ConfigPPO.policy.activation).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nightmare_rl_amd.envs.helpers import get_load_path  # noqa: E402
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO  # noqa: E402
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env  # noqa: E402
from nightmare_rl_amd.policy import ActorMLP, flat_params_from_state_dict  # noqa: E402


def actor_from_checkpoint(path, device, activation=None):
    """ActorMLP with the weights of `actor.<2i>.weight/bias` (rsl_rl ActorCritic layout) + the learned action std. activation: the
    networks' hidden activation (None: the training config's, NightmareV3ConfigPPO.policy.activation)."""
    activation = activation or NightmareV3ConfigPPO.policy.activation
    sd = torch.load(path, map_location="cpu")["model_state_dict"]
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("actor.") and k.endswith(".weight")})
    dims = [sd[f"actor.{idx[0]}.weight"].shape[1]] + [sd[f"actor.{i}.weight"].shape[0] for i in idx]
    net = ActorMLP(dims, activation=activation)
    for layer, i in zip(net.layers, idx):
        layer.weight.data.copy_(sd[f"actor.{i}.weight"])
        layer.bias.data.copy_(sd[f"actor.{i}.bias"])
    net = net.to(device)
    net.mark_dirty()
    return net, sd["std"].to(device)


def play_one_launch(a, path, env, cfg, dev):
    """The loop of main() as launches of --launch-steps steps (NightmareV3Env.policy_play); the summary comes from the tensors the kernel
    keeps: running returns, per-env sum / number of finished returns. The sum of all rewards up to a step is (finished returns + running
    returns), so a launch boundary 200 steps before the end gives the 'last 200 steps' figure without a per-step read."""
    from nightmare_rl_amd import _lib
    flat, dims = flat_params_from_state_dict(torch.load(path, map_location="cpu")["model_state_dict"], dev)
    if not _lib.load().nm_play_supported((_lib.C.c_int32 * len(dims))(*dims), len(dims) - 1, _lib.activation_code(a.activation)):
        raise SystemExit(f"--one-launch: no play kernel for an actor of shape {dims} (use the per-step path)")
    if a.cmd is not None:
        if a.cmd[1] != 0.0:
            raise SystemExit("--one-launch --cmd: VY must be 0 (the env commands no lateral velocity)")
        env.set_fixed_commands((a.cmd[0], a.cmd[2]))
    env.reset()
    N = a.envs
    z = lambda n: torch.zeros(n, device=dev)
    stats = dict(cur_ret=z(N), cur_len=z(N), fin=z(3), ret_sum=z(N), ret_cnt=z(N))
    chunk = a.launch_steps or int(env.max_episode_length)
    if chunk < 1:
        raise SystemExit("--launch-steps must be at least 1")
    total = lambda: float(stats["ret_sum"].double().sum() + stats["cur_ret"].double().sum())
    tail0, before_tail, done = max(a.steps - 200, 0), 0.0, 0
    while done < a.steps:
        k = min(chunk, a.steps - done, tail0 - done if done < tail0 else a.steps)
        env.policy_play(k, flat, deterministic=a.deterministic, seed=a.seed, activation=a.activation, stats=stats)
        done += k
        if done == tail0:
            before_tail = total()
    tot = total()
    ndone, ret_sum = int(stats["ret_cnt"].sum()), float(stats["ret_sum"].double().sum())
    print(f"checkpoint {path}: {a.envs} robots x {a.steps} steps, decimation {cfg.control.decimation}, "
          f"{'mean' if a.deterministic else 'sampled'} actions")
    print(f"  mean reward per step {tot / (N * a.steps):.4f} (last 200 steps {(tot - before_tail) / (N * (a.steps - tail0)):.4f}); episodes finished {ndone}"
          + (f", mean return {ret_sum / ndone:.2f}" if ndone else ""))
    if "episode" in env.extras:
        print("  last episode statistics:", {k: round(float(v), 4) for k, v in env.extras["episode"].items()})
    print("  env counters:", env.counters())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint", nargs="?", default=None)
    ap.add_argument("--log-root", default="logs/nightmare_v3")
    ap.add_argument("-e", "--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1300)
    ap.add_argument("--decimation", type=int, default=None, help="physics substeps per policy step (reference play.py:23 uses 4, the env 2)")
    ap.add_argument("--deterministic", action="store_true", help="act_inference (mean action) instead of upstream's sampled nn.act")
    ap.add_argument("--cmd", type=float, nargs=3, default=None, metavar=("VX", "VY", "YAW"), help="fixed velocity command (default: the env's own resampling)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--activation", default=NightmareV3ConfigPPO.policy.activation,
                    help="hidden activation the checkpoint was trained with (not stored in it; default: the training config's)")
    ap.add_argument("--one-launch", action="store_true", help="policy and env step inside one kernel, --launch-steps steps per launch (nm_play)")
    ap.add_argument("--launch-steps", type=int, default=None, help="steps per launch with --one-launch (default: one episode)")
    ap.add_argument("--record-states", default=None, metavar="DIR", help="write upstream's state log of env 0 (pickle files) into DIR")
    ap.add_argument("--push-interval-s", type=float, default=0.0, help="push every robot's base velocity every S seconds (0 = off, the default)")
    ap.add_argument("--push-vel", type=float, default=1.0, help="max |vx|, |vy| of a push in m/s")
    ap.add_argument("--friction-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="per-env sliding friction, drawn once from U[LO, HI) (default: 1.0)")
    ap.add_argument("--added-mass-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), dest="added_mass_range",
                    help="per-env point mass on the base body in kg (may be negative), drawn once from U[LO, HI) (default: none)")
    ap.add_argument("--com-range", type=float, default=None, metavar="R", dest="com_range",
                    help="where the added mass sits: each coordinate in the base body frame drawn once from U[-R, R) m (default: the base origin)")
    ap.add_argument("--latency-range", type=int, nargs=2, default=None, metavar=("LO", "HI"), dest="latency_range",
                    help="per-env actuation latency in physics substeps, drawn once from the integers LO..HI, at most 3 x decimation (default: none)")
    ap.add_argument("--gain-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="per-env multipliers of the servo stiffness and damping, each drawn once from U[LO, HI) (default: 1.0)")
    ap.add_argument("--action-rate-limit", type=float, default=None, metavar="R", dest="action_rate_limit",
                    help="the servo target may move at most R rad per control step (upstream's commented-out control.action_rate_limit = 0.08; default: no limit)")
    ap.add_argument("--d-gain", type=float, default=None, metavar="D", dest="d_gain",
                    help="damping D on the joint velocity in the servo command (upstream's commented-out control.d_gain = 0.05; default: 0)")
    ap.add_argument("--torque-limit", type=float, default=None, metavar="F", dest="torque_limit",
                    help="every servo delivers at most F N m (MuJoCo's actuator forcerange; default: no limit)")
    ap.add_argument("--resample-on-reset", type=int, nargs="?", const=1024, default=None, metavar="P", dest="resample_on_reset",
                    help="re-draw every per-env range above at every reset of an env, from a pool of P rows per kind (default P: 1024), instead of once")
    a = ap.parse_args()
    path = a.checkpoint or get_load_path(a.log_root)
    dev = torch.device("cuda", 0)
    cfg = NightmareV3Config()
    cfg.env.num_envs = a.envs
    if a.decimation is not None:
        cfg.control.decimation = a.decimation
    if a.record_states is not None:
        cfg.viewer.record_states = True
    if a.push_interval_s > 0 or a.friction_range or a.gain_range or a.added_mass_range or a.com_range is not None or a.latency_range:
        class domain_rand:      # the optional class NightmareV3Env reads
            push_robots, push_interval_s, max_push_vel_xy = a.push_interval_s > 0, a.push_interval_s, a.push_vel
            randomize_friction, friction_range = a.friction_range is not None, a.friction_range
            randomize_gains = a.gain_range is not None
            stiffness_multiplier_range = damping_multiplier_range = a.gain_range
            randomize_base_mass, added_mass_range = a.added_mass_range is not None, a.added_mass_range
            randomize_com_displacement = a.com_range is not None
            com_displacement_range = None if a.com_range is None else (-a.com_range, a.com_range)
            randomize_action_latency, action_latency_range = a.latency_range is not None, a.latency_range
            resample_on_reset = a.resample_on_reset is not None
            resample_pool_size = a.resample_on_reset if a.resample_on_reset is not None else 1024
        cfg.domain_rand = domain_rand
    if a.action_rate_limit is not None:      # upstream's own names (reference envs/nightmare_v3_config.py:37-38)
        cfg.control.action_rate_limit = a.action_rate_limit
    if a.d_gain is not None:
        cfg.control.d_gain = a.d_gain
    if a.torque_limit is not None:
        cfg.control.torque_limit = a.torque_limit
    env = NightmareV3Env(cfg, device=dev, seed=a.seed, **({"log_dir": a.record_states} if a.record_states is not None else {}))
    print(f"push perturbations: every {env.push_interval} steps, |v| < {env.max_push_vel_xy} m/s" if env.push_interval else "push perturbations: off")
    if a.friction_range or a.gain_range:
        print(f"per-env friction range {a.friction_range or 'off'}, gain multiplier range {a.gain_range or 'off'}")
    if a.one_launch:
        return play_one_launch(a, path, env, cfg, dev)
    net, std = actor_from_checkpoint(path, dev, a.activation)
    torch.manual_seed(a.seed)
    obs, _ = env.reset()
    ret = torch.zeros(a.envs, device=dev)
    done_returns, ndone, track = [], 0, []
    for t in range(a.steps):
        if a.cmd is not None:
            env.set_buffers(commands=np.tile(np.array(a.cmd, np.float64), (a.envs, 1)))
        mean = net(obs)
        act = mean if a.deterministic else mean + std * torch.randn_like(mean)
        obs, _, rew, done, extras = env.step(act)
        ret += rew
        d = done > 0
        if bool(d.any()):
            done_returns += ret[d].tolist()
            ndone += int(d.sum())
            ret[d] = 0
        track.append(float(rew.mean()))
    print(f"checkpoint {path}: {a.envs} robots x {a.steps} steps, decimation {cfg.control.decimation}, "
          f"{'mean' if a.deterministic else 'sampled'} actions")
    print(f"  mean reward per step {np.mean(track):.4f} (last 200 steps {np.mean(track[-200:]):.4f}); episodes finished {ndone}"
          + (f", mean return {np.mean(done_returns):.2f}" if done_returns else ""))
    if "episode" in extras:
        print("  last episode statistics:", {k: round(float(v), 4) for k, v in extras["episode"].items()})
    print("  env counters:", env.counters())


if __name__ == "__main__":
    main()
