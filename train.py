#!/usr/bin/env python
"""train.py - the reference's training entry point (reference train.py:1-54) on the MI355X backend.
Same flags (-r resume, -v render [rejected: no viewer], -n num_threads [accepted, unused], -e envs, -p resume_path) plus
--iters / --seed / --gpus / --push-interval-s / --push-vel / --wrench-interval-s / --wrench-duration-s / --wrench-force / --wrench-torque / --friction-range / --gain-range / --reset-dof-pos / --reset-vel. Multi-GPU: `python train.py --gpus G -e <total envs>` (starts its G ranks as child processes) or
`python -m torch.distributed.run --nproc-per-node G train.py -e <total envs>`."""
import argparse
import datetime
import os

import torch

from nightmare_rl_amd.distributed import shard_range
from nightmare_rl_amd.envs.helpers import class_to_dict, get_load_path
from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config, NightmareV3ConfigPPO
from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
from nightmare_rl_amd.rl import OnPolicyRunner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-r", "--resume", action="store_true", default=False, dest="resume")
    ap.add_argument("-v", "--render", action="store_true", default=False, dest="render")
    ap.add_argument("-n", "--num_threads", type=int, default=1, dest="num_threads")
    ap.add_argument("-e", "--envs", type=int, default=2048, dest="num_envs")
    ap.add_argument("-p", "--resume_path", type=str, default=None, dest="resume_path")
    ap.add_argument("--iters", type=int, default=None, help="learning iterations (default: cfg.runner.max_iterations)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--record-states", action="store_true", default=False, dest="record_states",
                    help="upstream's viewer.record_states: pickle env 0's states into the run's log directory whenever it resets (envs/nightmare_v3_env.py:261-272)")
    ap.add_argument("--push-interval-s", type=float, default=0.0, dest="push_interval_s",
                    help="push perturbations: seconds between two pushes of every robot's base velocity (0 = off, the default)")
    ap.add_argument("--push-vel", type=float, default=1.0, dest="push_vel", help="push perturbations: max |vx|, |vy| of a push in m/s")
    ap.add_argument("--wrench-interval-s", type=float, default=0.0, dest="wrench_interval_s",
                    help="external wrench on the base: seconds between the starts of two windows with a random force and torque (0 = off, the default)")
    ap.add_argument("--wrench-duration-s", type=float, default=None, dest="wrench_duration_s",
                    help="external wrench: seconds a window lasts, at most the interval (default: the whole interval)")
    ap.add_argument("--wrench-force", type=float, default=None, metavar="F", dest="wrench_force",
                    help="external wrench: each component of the force drawn from U[-F, F) N per window (default: 0)")
    ap.add_argument("--wrench-torque", type=float, default=None, metavar="T", dest="wrench_torque",
                    help="external wrench: each component of the torque drawn from U[-T, T) N m per window (default: 0)")
    ap.add_argument("--friction-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), dest="friction_range",
                    help="per-env sliding friction, drawn once from U[LO, HI) (default: 1.0 in every env)")
    ap.add_argument("--added-mass-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), dest="added_mass_range",
                    help="per-env point mass on the base body in kg (may be negative), drawn once from U[LO, HI) (default: none)")
    ap.add_argument("--com-range", type=float, default=None, metavar="R", dest="com_range",
                    help="where the added mass sits: each coordinate in the base body frame drawn once from U[-R, R) m (default: the base origin)")
    ap.add_argument("--latency-range", type=int, nargs=2, default=None, metavar=("LO", "HI"), dest="latency_range",
                    help="per-env actuation latency in physics substeps, drawn once from the integers LO..HI, at most 3 x decimation (default: none)")
    ap.add_argument("--obs-latency-range", type=int, nargs=2, default=None, metavar=("LO", "HI"), dest="obs_latency_range",
                    help="sensor model: per-env observation latency of the IMU and of the joint feedback in whole env steps, each drawn once from "
                         "the integers LO..HI, at most 3 (default: none)")
    ap.add_argument("--sensor-bias", type=str, nargs="+", default=None, metavar="KIND=MAX", dest="sensor_bias",
                    help="sensor model: per-env constant observation offsets, each column of KIND (lin_vel, ang_vel, gravity, dof_pos, dof_vel) drawn "
                         "once from U[-MAX, MAX) in physical units (default: none)")
    ap.add_argument("--reset-dof-pos", type=float, default=0.0, metavar="R", dest="reset_dof_pos",
                    help="randomised reset states: every reset draws each joint angle from U[-R, R) rad around the default pose (0 = off, the default)")
    ap.add_argument("--reset-vel", type=float, default=0.0, metavar="V", dest="reset_vel",
                    help="randomised reset states: every reset draws the base's linear (m/s) and angular (rad/s) velocity and the joint "
                         "velocities (rad/s) from U[-V, V) (0 = off, the default)")
    ap.add_argument("--gain-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), dest="gain_range",
                    help="per-env multipliers of the servo stiffness (p_gain) and damping (kv), each drawn once from U[LO, HI) (default: 1.0)")
    ap.add_argument("--action-rate-limit", type=float, default=None, metavar="R", dest="action_rate_limit",
                    help="the servo target may move at most R rad per control step (upstream's commented-out control.action_rate_limit = 0.08; default: no limit)")
    ap.add_argument("--d-gain", type=float, default=None, metavar="D", dest="d_gain",
                    help="damping D on the joint velocity in the servo command (upstream's commented-out control.d_gain = 0.05; default: 0)")
    ap.add_argument("--torque-limit", type=float, default=None, metavar="F", dest="torque_limit",
                    help="every servo delivers at most F N m (MuJoCo's actuator forcerange; default: no limit)")
    ap.add_argument("--resample-on-reset", type=int, nargs="?", const=1024, default=None, metavar="P", dest="resample_on_reset",
                    help="re-draw every per-env range above at every reset of an env, from a pool of P rows per kind (default P: 1024), instead of once")
    ap.add_argument("--privileged-obs", action="store_true", default=False, dest="privileged_obs",
                    help="asymmetric actor-critic: the critic also sees every env's drawn physics parameters (friction, gains, payload, latency, "
                         "gravity, servo, torque limit, wrench) and the base height; the actor keeps the 66 observations (default: off)")
    ap.add_argument("--privileged-rollout", action="store_true", default=False, dest="privileged_rollout",
                    help="with privileged critic observations, collect the rollout as one launch with the policy in the env's wave instead of "
                         "per-step launches; implies --privileged-obs (default: off)")
    ap.add_argument("--gpus", type=int, default=None, help="ranks (one per GPU); without torch.distributed.run, train.py starts them itself")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus is not None and args.gpus > 1:
        # called directly: the ranks become child processes of this one, which has not touched the GPU (and leaves with their status)
        import sys
        from nightmare_rl_amd.distributed import self_launch
        raise SystemExit(self_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("NM_DIST_BACKEND", "nccl")   # gloo: rehearse the multi-rank path on a box with fewer GPUs than ranks
    if backend != "nccl":
        local_rank %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    if world > 1 or os.environ.get("NM_FORCE_DATA_PARALLEL") == "1":      # (the switch: one rank down the multi-rank path, for a kernel trace)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    log_root = "logs/nightmare_v3/"
    log_dir = f"logs/nightmare_v3/{datetime.datetime.now()}/"
    cfg_class = NightmareV3Config
    if args.privileged_obs or args.privileged_rollout:
        class cfg_class(NightmareV3Config):      # the optional attribute NightmareV3Env reads
            class env(NightmareV3Config.env):
                privileged_obs = True
    cfg, train_cfg = cfg_class(), NightmareV3ConfigPPO()
    cfg.viewer.render = args.render
    cfg.viewer.record_states = bool(args.record_states) and rank == 0        # one log: rank 0's env 0
    if args.reset_dof_pos < 0 or args.reset_vel < 0:
        ap.error("--reset-dof-pos and --reset-vel must not be negative")
    reset_noise = args.reset_dof_pos > 0 or args.reset_vel > 0
    if args.wrench_interval_s < 0:
        ap.error("--wrench-interval-s must not be negative")
    if args.wrench_interval_s > 0 and args.wrench_force is None and args.wrench_torque is None:
        ap.error("--wrench-interval-s needs --wrench-force or --wrench-torque")
    sensor_bias = {}
    for item in args.sensor_bias or []:
        kind, sep, val = item.partition("=")
        try:
            sensor_bias[kind] = float(val)
        except ValueError:
            sep = ""
        if not sep or kind not in ("lin_vel", "ang_vel", "gravity", "dof_pos", "dof_vel"):
            ap.error(f"--sensor-bias takes KIND=MAX with KIND one of lin_vel, ang_vel, gravity, dof_pos, dof_vel, got {item!r}")
    if (args.push_interval_s > 0 or args.wrench_interval_s > 0 or args.friction_range or args.gain_range or args.added_mass_range or args.com_range is not None or args.latency_range
            or reset_noise or args.obs_latency_range or sensor_bias):
        class domain_rand:      # the optional class NightmareV3Env reads
            push_robots, push_interval_s, max_push_vel_xy = args.push_interval_s > 0, args.push_interval_s, args.push_vel
            external_wrench, wrench_interval_s = args.wrench_interval_s > 0, args.wrench_interval_s
            wrench_duration_s = args.wrench_duration_s if args.wrench_duration_s is not None else args.wrench_interval_s
            max_wrench_force, max_wrench_torque = args.wrench_force, args.wrench_torque
            randomize_friction, friction_range = args.friction_range is not None, args.friction_range
            randomize_gains = args.gain_range is not None
            stiffness_multiplier_range = damping_multiplier_range = args.gain_range
            randomize_base_mass, added_mass_range = args.added_mass_range is not None, args.added_mass_range
            randomize_com_displacement = args.com_range is not None
            com_displacement_range = None if args.com_range is None else (-args.com_range, args.com_range)
            randomize_action_latency, action_latency_range = args.latency_range is not None, args.latency_range
            randomize_obs_latency = args.obs_latency_range is not None
            imu_latency_range = joint_latency_range = args.obs_latency_range
            randomize_sensor_bias = bool(sensor_bias)
            randomize_reset_state = reset_noise
            reset_dof_pos_range = (-args.reset_dof_pos, args.reset_dof_pos)
            reset_base_lin_vel_range = reset_base_ang_vel_range = reset_dof_vel_range = (-args.reset_vel, args.reset_vel)
            resample_on_reset = args.resample_on_reset is not None
            resample_pool_size = args.resample_on_reset if args.resample_on_reset is not None else 1024
        domain_rand.sensor_bias = sensor_bias
        cfg.domain_rand = domain_rand
    if args.action_rate_limit is not None:      # upstream's own names (reference envs/nightmare_v3_config.py:37-38)
        cfg.control.action_rate_limit = args.action_rate_limit
    if args.d_gain is not None:
        cfg.control.d_gain = args.d_gain
    if args.torque_limit is not None:
        cfg.control.torque_limit = args.torque_limit
    lo, hi = shard_range(args.num_envs, rank, world)
    cfg.env.num_envs = hi - lo
    train_cfg.runner.resume = args.resume
    if args.privileged_rollout:
        train_cfg.runner.privileged_rollout = True
    seed = train_cfg.seed if args.seed is None else args.seed
    torch.manual_seed(seed + rank)
    env = NightmareV3Env(cfg, log_dir=log_dir, num_threads=args.num_threads, device=f"cuda:{local_rank}", seed=seed, env_id_offset=lo)
    if rank == 0:
        print(f"push perturbations: every {env.push_interval} steps, |v| < {env.max_push_vel_xy} m/s" if env.push_interval else "push perturbations: off", flush=True)
        if env.wrench_interval:
            iv, du, mf, mt, _ = env.wrench_schedule()
            print(f"external wrench: every {iv} steps for {du} steps, |F| < {mf[0]} N, |tau| < {mt[0]} N m per axis", flush=True)
        if env.sensor_model()["on"]:
            print(f"sensor model: observation latency {args.obs_latency_range or 'off'} env steps, bias maxima {sensor_bias or 'off'}", flush=True)
        if reset_noise:
            print(f"randomised reset states: joint angles +-{args.reset_dof_pos} rad, velocities +-{args.reset_vel}", flush=True)
        if args.friction_range or args.gain_range:
            print(f"per-env friction range {args.friction_range or 'off'}, gain multiplier range {args.gain_range or 'off'}", flush=True)
    runner = OnPolicyRunner(env, class_to_dict(train_cfg), log_dir=log_dir, device=f"cuda:{local_rank}")
    if train_cfg.runner.resume:
        path = get_load_path(args.resume_path or log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
        print(f"Loading model from: {path}")
        runner.load(path)
    runner.learn(num_learning_iterations=args.iters if args.iters is not None else train_cfg.runner.max_iterations, init_at_random_ep_len=True)
    counters = env.counters()                                # contacts dropped (provably 0), MuJoCo-style bad-state resets, search fallbacks
    if world > 1:
        # every rank must hold the same policy after the data-parallel updates: the largest difference to rank 0's parameters, and the
        # env counters summed over the shards
        dev = f"cuda:{local_rank}"
        flat = torch.cat([p.detach().reshape(-1).float() for p in runner.alg.actor_critic.parameters()]).to(dev)
        ref = flat.clone()
        dist.broadcast(ref, 0)
        diff = (flat - ref).abs().max().reshape(1)
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
        c = torch.tensor([counters[k] for k in sorted(counters)], device=dev, dtype=torch.float64)
        dist.all_reduce(c)
        counters = {k: int(v) for k, v in zip(sorted(counters), c.tolist())}
        if rank == 0:
            print(f"replicas: {world} ranks, max |parameter difference to rank 0| = {float(diff):.3e}", flush=True)
    if rank == 0:
        print("env counters:", counters, flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
