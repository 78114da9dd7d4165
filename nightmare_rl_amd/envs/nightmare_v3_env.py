"""NightmareV3Env: the reference's vectorised env surface (reference envs/nightmare_v3_env.py:26-396) over the
MI355X-native step kernel. Same constructor, attributes and return tuples; state lives in HBM and every call is
asynchronous on the current torch stream.

Differences a caller can observe (all documented in DESIGN.md):
  * returned tensors are views of persistent device buffers (the reference returns fresh CPU tensors, :311). The observation
    returned by step t stays untouched through step t+1 (two buffers, alternating), so a caller that keeps it across the next
    env.step and copies it afterwards - rsl_rl's PPO.act -> env.step -> storage.add_transitions - stores what the policy saw;
    rewards / dones / time_outs are valid until the next step()
  * commands come from a counter-based generator keyed by (seed, global env id) instead of numpy's global RNG (:327-330)
  * no viewer (`cfg.viewer.render` must be False); `cfg.viewer.record_states` writes the reference's pickle log (:261-272)
    at the price of one device sync per step() - or one per K-step launch (policy_rollout, policy_play), which keep the log on the device
  * observation noise (`cfg.noise.add_noise`, :304-305) draws from the same counter generator; `cfg.noise.layout`
    chooses between the reference's noise_scale_vec (written for a 12-dof robot, :113-119) and the 18-dof one
  * an OPTIONAL `cfg.domain_rand` (push_robots, push_interval_s, max_push_vel_xy - the names of legged_gym-shaped config trees; the
    reference has none) switches on push perturbations of the base velocity (set_push); the observation returned by the step before
    a push does not show it
  * the same optional class may carry randomize_friction / friction_range and randomize_gains / stiffness_multiplier_range /
    damping_multiplier_range: per-env sliding friction and servo gains, drawn once at construction (set_env_params, draw_env_params)
  * and randomize_base_mass / added_mass_range, randomize_com_displacement / com_displacement_range: a per-env point mass on the base
    body, compiled into the env's model constants (set_base_payload, draw_base_payload), drawn once at construction
  * and randomize_action_latency / action_latency_range (whole physics substeps): per-env actuation latency - the servo targets lag the
    policy's actions (set_action_latency, draw_action_latency), drawn once at construction
  * and randomize_reset_state with reset_base_height_range / reset_dof_pos_range / reset_base_lin_vel_range / reset_base_ang_vel_range /
    reset_dof_vel_range: every reset draws the base height, the joint angles and all velocities afresh around qpos0 / zero
    (set_reset_noise), from the first reset() on
  * and randomize_gravity / gravity_range, randomize_slope / slope_range, gravity_observed: a per-env gravity vector - a floor inclined
    by theta is a level floor under a gravity tilted by theta - drawn once at construction (set_gravity, draw_gravity)
  * an OPTIONAL `cfg.control.action_rate_limit` / `cfg.control.d_gain` - the two lines upstream's config keeps commented out
    (reference envs/nightmare_v3_config.py:37-38) - switch on the servo target model: a slew-rate limit on the servo target and a
    damping term (set_servo; reference envs/nightmare_v3_env.py:97,187-188, commented out as well). cfg.domain_rand may carry
    randomize_action_rate_limit / action_rate_limit_range and randomize_d_gain / d_gain_range, drawn once at construction (draw_servo)
  * an OPTIONAL `cfg.control.torque_limit` (N m; a scalar or one value each for the coxa, femur and tibia servos) bounds the servo
    torque as MuJoCo's actuator forcerange does (set_torque_limit); cfg.domain_rand may carry randomize_torque_limit /
    torque_limit_range, drawn once at construction (draw_torque_limit). The reference has neither: its servos are ideal
  * and cfg.domain_rand.resample_on_reset / resample_pool_size: every per-env kind whose randomize_* switch is on is then re-drawn at
    every reset of an env - in step(), reset_idx, policy_rollout, policy_play and step_tape alike - from a pool of rows filled from the
    same ranges (set_reset_pool), instead of being drawn once
  * and external_wrench with wrench_interval_s / wrench_duration_s / max_wrench_force / max_wrench_torque: a random force and torque on
    the base body, MuJoCo's xfrc_applied, held for wrench_duration_s out of every wrench_interval_s (set_wrench_schedule; a constant
    wrench: set_base_wrench). It acts through the physics and the contact solver, unlike a push; the reference applies none
  * and randomize_obs_latency with imu_latency_range / joint_latency_range (whole env steps, at most 3), randomize_sensor_bias with
    sensor_bias (maxima per kind, physical units): the per-env sensor model - the IMU and joint columns of the observation arrive late
    and carry a constant offset, in step(), policy_rollout, policy_play and step_tape alike (set_sensor_model, draw_sensor_model),
    drawn once at construction; the commands and the previous actions are never touched, and true_observations() is the step's own row
"""
import ctypes as C
import numpy as np
import torch

from .. import _lib
from . import privileged
from .helpers import class_to_dict
from .nightmare_v3_config import NightmareV3Config
from .state_log import ROW as _LOG_ROW, StateLog


def push_config(cfg, dt):
    """(interval_steps, max_vel_xy) of the optional cfg.domain_rand, (0, 0.0) when the class is missing or push_robots is false.
    push_interval_s is converted with the env's dt (whole steps, rounded down; 1e-9 of a step absorbs the division's rounding, so that
    0.048 s at dt 0.016 is 3 steps); an interval below one step or a negative / non-finite velocity is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    if dr is None or not getattr(dr, "push_robots", False):
        return 0, 0.0
    steps = float(dr.push_interval_s) / float(dt) + 1e-9
    if not steps >= 1:
        raise ValueError("cfg.domain_rand.push_interval_s must be at least one env step (dt)")
    vel = float(dr.max_push_vel_xy)
    if not (vel >= 0 and np.isfinite(vel)):
        raise ValueError("cfg.domain_rand.max_push_vel_xy must be finite and >= 0")
    if steps >= 2 ** 31:
        raise ValueError("cfg.domain_rand.push_interval_s is more than 2^31 env steps")
    return int(steps), vel


def wrench_config(cfg, dt):
    """(interval_steps, duration_steps, max_force, max_torque) of the optional cfg.domain_rand, None when the class is missing or
    external_wrench is false. wrench_interval_s and wrench_duration_s are converted with the env's dt by push_config's rule (whole steps,
    rounded down; 1e-9 of a step absorbs the division's rounding); max_wrench_force (N) and max_wrench_torque (N m) are each a scalar - all
    three axes - or three values, finite and >= 0, and at least one of the two must be given (the other is then zero). An interval or a
    duration below one step, a duration above the interval, or a bad maximum is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    if dr is None or not getattr(dr, "external_wrench", False):
        return None
    steps = []
    for name in ("wrench_interval_s", "wrench_duration_s"):
        v = getattr(dr, name, None)
        if v is None:
            raise ValueError(f"cfg.domain_rand.external_wrench needs {name}")
        s = float(v) / float(dt) + 1e-9
        if not s >= 1:
            raise ValueError(f"cfg.domain_rand.{name} must be at least one env step (dt)")
        if s >= 2 ** 31:
            raise ValueError(f"cfg.domain_rand.{name} is more than 2^31 env steps")
        steps.append(int(s))
    if steps[1] > steps[0]:
        raise ValueError("cfg.domain_rand.wrench_duration_s must not exceed wrench_interval_s")
    maxima = []
    for name in ("max_wrench_force", "max_wrench_torque"):
        v = getattr(dr, name, None)
        if v is None:
            maxima.append(None)
            continue
        try:
            a = np.asarray(v, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"cfg.domain_rand.{name} must be a number or three numbers") from None
        if a.size not in (1, 3):
            raise ValueError(f"cfg.domain_rand.{name} must be a number or three numbers (x, y, z)")
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"cfg.domain_rand.{name} must be finite and >= 0")
        maxima.append([float(x) for x in np.broadcast_to(a, (3,))])
    if maxima[0] is None and maxima[1] is None:
        raise ValueError("cfg.domain_rand.external_wrench needs max_wrench_force or max_wrench_torque")
    return steps[0], steps[1], maxima[0] or [0.0] * 3, maxima[1] or [0.0] * 3


def _range(dr, name, lowest=None, strict=False, whole=False):
    """cfg.domain_rand.<name> as a pair (lo, hi) of finite numbers lo <= hi, or None where there is none. lowest: lo's lower bound
    (strict: lo must be above it); whole: whole numbers, returned as integers. Anything else is a ValueError."""
    r = getattr(dr, name, None)
    if r is None:
        return None
    try:
        lo, hi = (float(x) for x in r)
    except (TypeError, ValueError):
        raise ValueError(f"cfg.domain_rand.{name} must be a pair (lo, hi)") from None
    bound = "" if lowest is None else f"{lowest} {'<' if strict else '<='} "
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi and (lowest is None or (lo > lowest if strict else lo >= lowest))
            and (not whole or (lo == int(lo) and hi == int(hi)))):
        raise ValueError(f"cfg.domain_rand.{name} must be {'whole substeps' if whole else 'finite'} with {bound}lo <= hi")
    return (int(lo), int(hi)) if whole else (lo, hi)


def _switched(dr, flag, name, **kw):
    """The range cfg.domain_rand.<name> where cfg.domain_rand.<flag> is set - a ValueError where it is missing - and None where it is not."""
    if not getattr(dr, flag, False):
        return None
    r = _range(dr, name, **kw)
    if r is None:
        raise ValueError(f"cfg.domain_rand.{flag} needs {name}")
    return r


def env_param_config(cfg):
    """(friction_range, stiffness_multiplier_range, damping_multiplier_range) of the optional cfg.domain_rand, each a (lo, hi) pair or None:
    what draw_env_params takes. randomize_friction needs friction_range; randomize_gains takes the multiplier ranges that are there (a
    missing one leaves that gain alone). A range that is not two finite numbers lo <= hi, a friction at or below 1e-5 or a negative
    multiplier is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)      # (a missing class reads as every switch off)
    st = da = None
    fr = _switched(dr, "randomize_friction", "friction_range", lowest=1e-5, strict=True)
    if getattr(dr, "randomize_gains", False):
        st, da = _range(dr, "stiffness_multiplier_range", 0.0), _range(dr, "damping_multiplier_range", 0.0)
        if st is None and da is None:
            raise ValueError("cfg.domain_rand.randomize_gains needs stiffness_multiplier_range or damping_multiplier_range")
    return fr, st, da


def payload_config(cfg):
    """(mass_range, com_range) of the optional cfg.domain_rand, each a (lo, hi) pair or None: what draw_base_payload takes.
    randomize_base_mass needs added_mass_range (kg, may be negative), randomize_com_displacement needs com_displacement_range (m, the
    same range for x, y and z in the base body frame). A range that is not two finite numbers lo <= hi is a ValueError; whether the
    heaviest negative mass is admissible is judged when the rows are derived (model/payload.py)."""
    dr = getattr(cfg, "domain_rand", None)
    return _switched(dr, "randomize_base_mass", "added_mass_range"), _switched(dr, "randomize_com_displacement", "com_displacement_range")


def latency_config(cfg):
    """(lo, hi) in whole physics substeps from the optional cfg.domain_rand, or None: what draw_action_latency takes.
    randomize_action_latency needs action_latency_range; a range that is not two integers 0 <= lo <= hi is a ValueError (the upper limit,
    three env steps, is the library's to judge: it depends on the decimation)."""
    return _switched(getattr(cfg, "domain_rand", None), "randomize_action_latency", "action_latency_range", lowest=0, whole=True)


def sensor_config(cfg):
    """(imu_latency_range, joint_latency_range, bias_max) of the sensor model from the optional cfg.domain_rand: what draw_sensor_model
    takes. Each range is a (lo, hi) pair of whole env steps or None, bias_max a dict {kind: maximum absolute offset in OBSERVATION units}
    or None. randomize_obs_latency needs imu_latency_range and/or joint_latency_range (integers 0 <= lo <= hi; the upper limit, three env
    steps, is the library's to judge); randomize_sensor_bias needs sensor_bias, a class or dict of any of lin_vel, ang_vel, gravity,
    dof_pos, dof_vel as finite maxima >= 0 in physical units, which are multiplied here by cfg.normalization.obs_scales (gravity, a unit
    vector's components, has no scale). Anything else is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    imu = joint = bias = None
    if getattr(dr, "randomize_obs_latency", False):
        imu = _range(dr, "imu_latency_range", lowest=0, whole=True)
        joint = _range(dr, "joint_latency_range", lowest=0, whole=True)
        if imu is None and joint is None:
            raise ValueError("cfg.domain_rand.randomize_obs_latency needs imu_latency_range or joint_latency_range")
    if getattr(dr, "randomize_sensor_bias", False):
        sb = getattr(dr, "sensor_bias", None)
        if sb is None:
            raise ValueError("cfg.domain_rand.randomize_sensor_bias needs sensor_bias")
        items = dict(sb) if isinstance(sb, dict) else {k: getattr(sb, k) for k in dir(sb) if not k.startswith("_")}
        unknown = sorted(set(items) - set(SENSOR_BIAS_KINDS))
        if unknown:
            raise ValueError(f"cfg.domain_rand.sensor_bias: unknown kinds {unknown} (known: {list(SENSOR_BIAS_KINDS)})")
        if not items:
            raise ValueError("cfg.domain_rand.sensor_bias must name at least one of " + ", ".join(SENSOR_BIAS_KINDS))
        scales = getattr(getattr(cfg, "normalization", None), "obs_scales", None)
        bias = {}
        for k, v in items.items():
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"cfg.domain_rand.sensor_bias.{k} must be a number") from None
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"cfg.domain_rand.sensor_bias.{k} must be finite and >= 0")
            bias[k] = v * (1.0 if k == "gravity" else float(getattr(scales, k)))
    return imu, joint, bias


SENSOR_BIAS_KINDS = ("lin_vel", "ang_vel", "gravity", "dof_pos", "dof_vel")      # nm_sensor.h sensor_col_kind: columns 0..2, 3..5, 6..8, 12..29, 30..47
SENSOR_MAX_DELAY, SENSOR_SLOTS = 3, 4                                            # nm_sensor.h kSensorMaxDelay, kSensorSlots


def servo_config(cfg):
    """(rate_range, d_gain_range) of the servo target model, each a (lo, hi) pair or None (= the default: no limit, no damping): what
    draw_servo takes. The optional cfg.control.action_rate_limit (rad per control step, > 0, inf = no limit) and cfg.control.d_gain
    (finite, >= 0) - upstream's own names, reference envs/nightmare_v3_config.py:37-38 - give every env that value, as the pair (v, v);
    cfg.domain_rand.randomize_action_rate_limit needs action_rate_limit_range (finite, 0 < lo <= hi), randomize_d_gain needs d_gain_range
    (finite, 0 <= lo <= hi), and a range takes the place of the value of cfg.control. Anything else is a ValueError."""
    ctl, dr = getattr(cfg, "control", None), getattr(cfg, "domain_rand", None)

    def value(name, ok, what):
        v = getattr(ctl, name, None)
        if v is None:
            return None
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"cfg.control.{name} must be a number") from None
        if not ok(v):
            raise ValueError(f"cfg.control.{name} must be {what}")
        return v

    rate = value("action_rate_limit", lambda v: v > 0, "above 0 (inf = no limit)")
    d_gain = value("d_gain", lambda v: np.isfinite(v) and v >= 0, "finite and >= 0")
    rr = _switched(dr, "randomize_action_rate_limit", "action_rate_limit_range", lowest=0.0, strict=True)
    dg = _switched(dr, "randomize_d_gain", "d_gain_range", lowest=0.0)
    if rr is None and rate is not None and np.isfinite(rate):
        rr = (rate, rate)
    if dg is None and d_gain is not None:
        dg = (d_gain, d_gain)
    return rr, dg


def torque_config(cfg):
    """(limit, limit_range) of the servo torque limit: `limit` three values (coxa, femur, tibia; N m, > 0, inf = no limit) from the
    optional cfg.control.torque_limit - a scalar gives all three - or None; `limit_range` a [3, 2] list of (lo, hi) pairs from the optional
    cfg.domain_rand.randomize_torque_limit / torque_limit_range - one pair (lo, hi) for all three joint types or three pairs, finite,
    0 < lo <= hi - or None; a range takes the place of the value. Anything else is a ValueError."""
    ctl, dr = getattr(cfg, "control", None), getattr(cfg, "domain_rand", None)
    limit = None
    v = getattr(ctl, "torque_limit", None)
    if v is not None:
        try:
            a = np.asarray(v, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("cfg.control.torque_limit must be a number or three numbers") from None
        if a.size not in (1, 3):
            raise ValueError("cfg.control.torque_limit must be a number or three numbers (coxa, femur, tibia)")
        if not (a > 0).all():
            raise ValueError("cfg.control.torque_limit must be above 0 (inf = no limit)")
        limit = [float(x) for x in np.broadcast_to(a, (3,))]
    rng = None
    if getattr(dr, "randomize_torque_limit", False):
        r = getattr(dr, "torque_limit_range", None)
        if r is None:
            raise ValueError("cfg.domain_rand.randomize_torque_limit needs torque_limit_range")
        try:
            a = np.asarray(r, np.float64)
        except (TypeError, ValueError):
            raise ValueError("cfg.domain_rand.torque_limit_range must be a pair (lo, hi) or three pairs") from None
        if a.shape == (2,):
            a = np.tile(a, (3, 1))
        if a.shape != (3, 2):
            raise ValueError("cfg.domain_rand.torque_limit_range must be a pair (lo, hi) or three pairs")
        if not (np.isfinite(a).all() and (a[:, 0] > 0).all() and (a[:, 0] <= a[:, 1]).all()):
            raise ValueError("cfg.domain_rand.torque_limit_range must be finite with 0 < lo <= hi")
        rng = a.tolist()
    return limit, rng


GRAVITY = 9.81      # m/s^2: the model's gravity and upstream's gravity_vec (reference envs/nightmare_v3_env.py:46)


def gravity_config(cfg):
    """(offset_range, tilt_range, observed) of the optional cfg.domain_rand: what draw_gravity takes, both ranges None where nothing is
    switched on. randomize_gravity needs gravity_range, (lo, hi) m/s^2 added to each component of g (legged_gym's names);
    randomize_slope needs slope_range, (lo, hi) rad with 0 <= lo <= hi < pi/2, the floor's inclination; gravity_observed (default True):
    whether the env layer sees g or keeps upstream's constant. Anything else is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    off = _switched(dr, "randomize_gravity", "gravity_range")
    tilt = _switched(dr, "randomize_slope", "slope_range", lowest=0.0)
    if tilt is not None and not tilt[1] < np.pi / 2:
        raise ValueError("cfg.domain_rand.slope_range must be finite with 0 <= lo <= hi < pi/2")
    observed = getattr(dr, "gravity_observed", True)
    if not isinstance(observed, (bool, np.bool_)):
        raise ValueError("cfg.domain_rand.gravity_observed must be True or False")
    return off, tilt, bool(observed)


def gravity_from_draw(offset, theta, phi):
    """g [n,3] in float64 of a floor inclined by theta towards azimuth phi, written in the floor's frame, plus a per-axis offset:
    9.81 (sin theta cos phi, sin theta sin phi, -cos theta) + offset."""
    offset, theta, phi = np.asarray(offset, np.float64), np.asarray(theta, np.float64), np.asarray(phi, np.float64)
    s = np.sin(theta)
    return GRAVITY * np.stack([s * np.cos(phi), s * np.sin(phi), -np.cos(theta)], axis=-1) + offset


RESET_NOISE_RANGES = ("reset_base_height_range", "reset_dof_pos_range", "reset_base_lin_vel_range", "reset_base_ang_vel_range",
                      "reset_dof_vel_range")


def reset_noise_config(cfg):
    """The five (lo, hi) ranges of randomised reset states from the optional cfg.domain_rand, in the order of RESET_NOISE_RANGES (what
    set_reset_noise takes), or None when the class is missing or randomize_reset_state is false. A missing range is (0, 0); the flag with
    no range at all, or a range that is not two finite numbers lo <= hi, is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    if not getattr(dr, "randomize_reset_state", False):
        return None
    if all(getattr(dr, n, None) is None for n in RESET_NOISE_RANGES):
        _switched(dr, "randomize_reset_state", " or ".join(RESET_NOISE_RANGES))       # (raises: the flag needs a range)
    return tuple(_range(dr, n) or (0.0, 0.0) for n in RESET_NOISE_RANGES)


RESET_POOL_KINDS = ("env_params", "base_payload", "action_latency", "gravity", "servo", "torque_limit")   # nmrows::Kind order
RESET_POOL_WIDTH = (4, 20, 1, 8, 4, 4)
RESET_POOL_MAX = 65536


def resample_config(cfg):
    """The pool size of the optional cfg.domain_rand.resample_on_reset, or None where the class is missing or the switch is false:
    every kind whose randomize_* switch is on is then re-drawn at every reset from a pool of resample_pool_size rows (default 1024,
    1..65536). A switch that is not True / False or a size that is not a whole number in that range is a ValueError."""
    dr = getattr(cfg, "domain_rand", None)
    on = getattr(dr, "resample_on_reset", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("cfg.domain_rand.resample_on_reset must be True or False")
    if not on:
        return None
    size = getattr(dr, "resample_pool_size", 1024)
    if isinstance(size, (bool, np.bool_)) or not isinstance(size, (int, np.integer)) or not 1 <= int(size) <= RESET_POOL_MAX:
        raise ValueError(f"cfg.domain_rand.resample_pool_size must be a whole number in 1..{RESET_POOL_MAX}")
    return int(size)


# ---- values -> rows: what the row setters and the reset pools (set_reset_pool) share. n: the number of rows (num_envs, or a pool's size);
# err: the caller's ValueError text for a wrong count
def per_row_values(x, n, dtype, err, device):
    """n values, or one scalar for every row, as a contiguous [n] tensor of `dtype` on `device`."""
    t = torch.as_tensor(x, dtype=dtype).detach().to(device)
    t = t.expand(n) if t.dim() == 0 else t.reshape(-1)
    if t.numel() != n:
        raise ValueError(err)
    return t.contiguous()


def env_param_columns(n, real, device, mu, p_gain, kv, err):
    """The three columns (mu, p_gain, kv) nm_set_env_params takes: [n] tensors, None = the default."""
    return [None if x is None else per_row_values(x, n, real, err, device) for x in (mu, p_gain, kv)]


def env_param_rows(cols, defaults, n, real, device):
    """[n, 4] rows (mu, p_gain, kv, pad) as the library forms them from the columns: a missing column holds its default."""
    rows = torch.zeros(n, 4, dtype=real, device=device)
    for j, (c, d) in enumerate(zip(cols, defaults)):
        rows[:, j] = d if c is None else c
    return rows


def vec3_rows(v, n, err):
    """[n, 3] float64 numpy from one [3] for every row or an [n, 3] array / tensor."""
    v = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    v = np.tile(v, (n, 1)) if v.ndim == 1 and v.size == 3 else v
    if v.shape != (n, 3):
        raise ValueError(err)
    return v


def payload_values(n, dm, r, err):
    """(dm [n], r [n, 3]) float64 numpy of a point mass per row: dm n values or a scalar, r [n, 3], one [3] for all or None = the origin."""
    dm = per_row_values(dm, n, torch.float64, err, "cpu").numpy()
    r = np.zeros(3) if r is None else np.asarray(r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else r, dtype=np.float64)
    r = np.tile(r, (n, 1)) if r.ndim == 1 else r.reshape(-1, 3)
    if r.shape != (n, 3):
        raise ValueError(err)
    return dm, r


def payload_body_rows(dm, r):
    """[n, 20] float64 body rows of the payloads (model/payload.py derives them; ValueError for what MuJoCo's compiler refuses)."""
    from ..model import payload
    return payload.payload_rows(dm, r)


def gravity_rows(n, g, gravity_vec, err):
    """[n, 8] float64 gravity rows: g[3], pad, gravity_vec[3] (None = g), pad."""
    rows = np.zeros((n, 8))
    rows[:, 0:3] = vec3_rows(g, n, err)
    rows[:, 4:7] = rows[:, 0:3] if gravity_vec is None else vec3_rows(gravity_vec, n, err)
    return rows


def servo_rows(n, real, device, rate_limit, d_gain, err):
    """[n, 4] servo rows (rate, d_gain, pad, pad): None = the column's default (inf, 0)."""
    rows = torch.zeros(n, 4, dtype=real, device=device)
    rows[:, 0] = float("inf") if rate_limit is None else per_row_values(rate_limit, n, real, err, device)
    if d_gain is not None:
        rows[:, 1] = per_row_values(d_gain, n, real, err, device)
    return rows


def torque_rows(n, real, device, limit, err):
    """[n, 4] torque-limit rows (coxa, femur, tibia, pad) from a scalar, 3 values, [n] or [n, 3]."""
    t = torch.as_tensor(limit, dtype=real).detach().to(device)
    if t.dim() == 0 or (t.dim() == 1 and t.numel() == 3):      # (with n == 3, three values are read as coxa, femur, tibia)
        t = t.expand(n, 3)
    elif t.dim() == 1 and t.numel() == n:
        t = t.reshape(n, 1).expand(n, 3)
    elif tuple(t.shape) != (n, 3):
        raise ValueError(err)
    rows = torch.zeros(n, 4, dtype=real, device=device)
    rows[:, :3] = t
    return rows


def latency_values(n, device, substeps, who):
    """[n] int32 delays from n integers or one integer for every row."""
    t = torch.as_tensor(substeps)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{who}: whole substeps (an integer per env)")
    return per_row_values(t, n, torch.int32, f"{who}: one delay per env (or one for all)", device)


def config_pools(cfg, seed, size, envp_default):
    """The reset pools of a config whose resample_on_reset is on: {kind: the keyword values set_reset_pool takes}, `size` rows each, for
    every kind whose randomize_* switch is on. Filled on the host in float64 from the ranges the *_config parsers return, with
    np.random.default_rng([seed, kind index]): no env id enters, so every rank of a sharded population builds the same pools.
    envp_default: (mu, p_gain, kv) the library runs with while friction / gains are off."""
    dr = getattr(cfg, "domain_rand", None)
    P = int(size)
    rng = [np.random.default_rng([int(seed), k]) for k in range(len(RESET_POOL_KINDS))]

    def uni(k, r, shape=None):
        return rng[k].uniform(r[0], r[1], P if shape is None else shape)

    pools = {}
    fr, st, da = env_param_config(cfg)
    if fr is not None or st is not None or da is not None:
        mu0, pg, kv0 = envp_default
        pools["env_params"] = dict(mu=None if fr is None else uni(0, fr), p_gain=None if st is None else uni(0, (pg * st[0], pg * st[1])),
                                   kv=None if da is None else uni(0, (kv0 * da[0], kv0 * da[1])))
    ma, co = payload_config(cfg)
    if ma is not None or co is not None:
        pools["base_payload"] = dict(dm=np.zeros(P) if ma is None else uni(1, ma), r=np.zeros((P, 3)) if co is None else uni(1, co, (P, 3)))
    lat = latency_config(cfg)
    if lat is not None:
        pools["action_latency"] = dict(substeps=rng[2].integers(lat[0], lat[1] + 1, P).astype(np.int32))
    off, tilt, observed = gravity_config(cfg)
    if off is not None or tilt is not None:
        o = np.zeros((P, 3)) if off is None else uni(3, off, (P, 3))
        theta = np.zeros(P) if tilt is None else uni(3, tilt)
        phi = np.zeros(P) if tilt is None else uni(3, (0.0, 2.0 * np.pi))
        pools["gravity"] = dict(g=gravity_from_draw(o, theta, phi), gravity_vec=None if observed else np.array([0.0, 0.0, -GRAVITY]))
    rr, dg = servo_config(cfg)
    if getattr(dr, "randomize_action_rate_limit", False) or getattr(dr, "randomize_d_gain", False):
        pools["servo"] = dict(rate_limit=None if rr is None else uni(4, rr), d_gain=None if dg is None else uni(4, dg))
    _, trange = torque_config(cfg)
    if trange is not None:
        a = np.asarray(trange, np.float64)
        pools["torque_limit"] = dict(limit=rng[5].uniform(a[:, 0], a[:, 1], (P, 3)))
    return pools


class NightmareV3Env:
    def __init__(self, cfg: NightmareV3Config, log_dir="/tmp/nightmare_v3/logs", num_threads=1, *, device=None, seed=0,
                 env_id_offset=0, dtype=torch.float32, lib=None):
        """lib: a loaded library object other than the shipped one (_lib.load_measure(): measurement scripts and one test only)."""
        self.cfg = cfg
        self.log_dir = log_dir
        self.thread_num = num_threads  # accepted for API parity; the GPU path has no host threads
        self.num_envs = int(cfg.env.num_envs)
        self.num_obs = int(cfg.env.num_obs)
        self.num_privileged_obs = self.num_obs  # reference :34
        self.num_actions = int(cfg.env.num_actions)
        if self.num_obs != _lib.NUM_OBS or self.num_actions != _lib.NUM_ACTIONS:
            raise ValueError("the compiled path is specialised for num_obs=66, num_actions=18")
        if cfg.viewer.render:
            raise ValueError("cfg.viewer.render is not available on the GPU path (set it to False)")
        if cfg.env.tibia_contact_mode not in (0, 1, 2) or cfg.env.body_contact_mode not in (0, 1, 2):
            raise ValueError("tibia/body_contact_mode: 0 do nothing, 1 penalize on contact, 2 terminate on contact")
        if not torch.cuda.is_available():
            raise _lib.NightmareHipError("NightmareV3Env needs a HIP device: there is no CPU path")
        L = lib if lib is not None else _lib.load()
        self._L = L
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise _lib.NightmareHipError(f"device must be a HIP device, got {dev}")
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_dof = 18
        self.gravity_vec = np.array([0., 0., -9.81])
        self.reward_scales = class_to_dict(cfg.rewards.scales)
        self.command_ranges = cfg.commands.ranges
        self.obs_scales = cfg.normalization.obs_scales
        # timestep 0.008 (reference models/nightmare_v3/mjmodel.xml:3) x decimation
        self.dt = 0.008 * cfg.control.decimation
        self.max_episode_length_s = cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)
        self.default_dof_pos = np.array(cfg.control.default_pos, dtype=np.float64)
        if int(cfg.commands.resampling_time / self.dt) < 1:
            raise ValueError("cfg.commands.resampling_time must be at least one env step (reference :235 takes a modulo by it)")
        push_steps, push_vel = push_config(cfg, self.dt)       # optional cfg.domain_rand: checked before anything is created
        envp_ranges = env_param_config(cfg)
        payload_ranges = payload_config(cfg)
        latency_range = latency_config(cfg)
        gravity_ranges = gravity_config(cfg)
        reset_ranges = reset_noise_config(cfg)
        servo_ranges = servo_config(cfg)
        torque_limit, torque_range = torque_config(cfg)
        resample_size = resample_config(cfg)
        wrench_sched = wrench_config(cfg, self.dt)
        sensor_ranges = sensor_config(cfg)
        # reward table: zero scales dropped, the rest x dt (reference :123-128). Every name the reference has a _reward_ function
        # for (:399-497) is compiled; a name without one (`collision`, `feet_stumble`, config :95-96) fails like upstream's getattr.
        names = [L.nm_reward_name(i).decode() for i in range(_lib.NUM_REWARDS)]
        for key in list(self.reward_scales.keys()):
            if self.reward_scales[key] == 0:
                self.reward_scales.pop(key)
            else:
                if key not in names:
                    raise AttributeError(f"'NightmareV3Env' object has no attribute '_reward_{key}'")
                self.reward_scales[key] *= self.dt
        self.reward_names = [n for n in self.reward_scales if n != "termination"]
        dp = list(cfg.control.default_pos)
        if any(abs(dp[i] - dp[i % 3]) > 0 for i in range(18)):
            raise NotImplementedError("default_pos must repeat per leg (coxa, femur, tibia)")
        c = _lib.NmConfig()
        L.nm_default_config(C.byref(c))
        c.decimation = int(cfg.control.decimation)
        c.p_gain = float(cfg.control.p_gain)
        c.action_scale = float(cfg.control.action_scale)
        for i in range(3):
            c.default_pos[i] = float(dp[i])
        c.clip_actions = float(cfg.normalization.clip_actions)
        c.clip_observations = float(cfg.normalization.clip_observations)
        c.obs_lin_vel, c.obs_ang_vel = float(self.obs_scales.lin_vel), float(self.obs_scales.ang_vel)
        c.obs_dof_pos, c.obs_dof_vel = float(self.obs_scales.dof_pos), float(self.obs_scales.dof_vel)
        c.episode_length_s = float(cfg.env.episode_length_s)
        c.resampling_time = float(cfg.commands.resampling_time)
        c.max_lin_vel_x, c.max_ang_vel = float(self.command_ranges.max_lin_vel_x), float(self.command_ranges.max_ang_vel)
        c.termination_contact_force = float(cfg.env.termination_contact_force)
        c.tracking_sigma = float(cfg.rewards.tracking_sigma)
        raw = class_to_dict(cfg.rewards.scales)
        for i, n in enumerate(names):
            c.reward_scales[i] = float(raw.get(n, 0.0))
        c.tibia_contact_mode, c.tibia_max_contact_force = int(cfg.env.tibia_contact_mode), float(cfg.env.tibia_max_contact_force)
        c.body_contact_mode, c.body_max_contact_force = int(cfg.env.body_contact_mode), float(cfg.env.body_max_contact_force)
        c.base_height_target, c.max_contact_force = float(cfg.rewards.base_height_target), float(cfg.rewards.max_contact_force)
        self._dtype = _lib.DTYPE_F64 if dtype == torch.float64 else _lib.DTYPE_F32
        self._real = torch.float64 if dtype == torch.float64 else torch.float32
        h = C.c_void_p()
        self._ck(L.nm_create(C.byref(c), self.num_envs, self.device.index or 0, int(seed), int(env_id_offset), self._dtype, C.byref(h)))
        self._h = h
        N, dev = self.num_envs, self.device
        # two observation buffers, written alternately: the tensor handed out by step t is not overwritten by step t+1
        self._obs_pair = torch.zeros((2, N, self.num_obs), dtype=torch.float32, device=dev)
        self._obs_idx = 0
        self.obs_buf = self._obs_pair[0]
        self.privileged_obs_buf = None
        # the privileged critic row (optional cfg.env.privileged_obs; envs/privileged.py; no reference line): [N, 66 + 23], gathered on the
        # device behind every step() and double-buffered like obs_buf. Off: the reference's surface (num_privileged_obs = num_obs, :34;
        # no privileged observations, :317-319)
        self.privileged_obs_has_obs_prefix = privileged.enabled(cfg)
        if self.privileged_obs_has_obs_prefix:
            self.num_privileged_obs = privileged.NUM_PRIVILEGED_OBS
            self._priv_pair = torch.zeros((2, N, self.num_privileged_obs), dtype=torch.float32, device=dev)
            self.privileged_obs_buf = self._priv_pair[0]
        self.rew_buf = torch.zeros(N, dtype=torch.float32, device=dev)
        self.reset_buf = torch.ones(N, dtype=torch.int64, device=dev)
        self.episode_length_buf = torch.zeros(N, dtype=torch.int64, device=dev)  # assignable, like the reference (:88)
        self.time_out_buf = torch.zeros(N, dtype=torch.float32, device=dev)
        self._to_bound = self.time_out_buf       # the tensor object the kernel's incremental time-out refresh is bound to
        self._ep_stats = torch.zeros(_lib.NUM_REWARDS, dtype=torch.float32, device=dev)
        self._stat_names = names
        self.extras = {}
        self.common_step_counter = 0
        # observation noise (reference :109-119, :304-305)
        self.noise_scale_vec = self._noise_scale_vec(cfg)
        self.add_noise = bool(cfg.noise.add_noise)
        if self.add_noise:
            self._ck(L.nm_set_observation_noise(h, self.noise_scale_vec.ctypes.data_as(C.c_void_p)))
        # push perturbations (optional cfg.domain_rand; no reference line)
        self.push_interval, self.max_push_vel_xy = 0, 0.0
        if push_steps:
            self.set_push(push_steps, push_vel)
        # per-env friction and servo gains (optional cfg.domain_rand; no reference line): drawn once, here, like legged_gym's friction
        # what the row setters hand to the library is copied stream-ordered: each kind's source tensors live here until its next call
        self._rows_keep = {}
        # the library's own defaults (the model's mu and kv, the config's p_gain): what it reports while the feature is off, read once here
        self._envp_default = tuple(float(v[0]) for v in self.env_params().values()) if hasattr(L, "nm_get_env_params") else None
        # re-drawn at every reset instead (cfg.domain_rand.resample_on_reset): the kinds whose randomize_* switch is on get a pool each,
        # installed before the first reset(), in place of their once-only draw below
        pools = config_pools(cfg, seed, resample_size, self._envp_default) if resample_size is not None else {}
        if "env_params" not in pools and any(r is not None for r in envp_ranges):
            self.draw_env_params(*envp_ranges)
        # per-env base payload (optional cfg.domain_rand; no reference line): drawn once, here
        self._payload = None
        if "base_payload" not in pools and any(r is not None for r in payload_ranges):
            self.draw_base_payload(*payload_ranges)
        # per-env actuation latency (optional cfg.domain_rand; no reference line): drawn once, here
        if "action_latency" not in pools and latency_range is not None:
            self.draw_action_latency(*latency_range)
        # per-env gravity vectors - slopes and gravity offsets (optional cfg.domain_rand; no reference line): drawn once, here
        if "gravity" not in pools and (gravity_ranges[0] is not None or gravity_ranges[1] is not None):
            self.draw_gravity(*gravity_ranges)
        # the servo target model (optional cfg.control.action_rate_limit / d_gain, reference config :37-38; optional cfg.domain_rand ranges):
        # set once, here, before the first reset()
        if "servo" not in pools and (servo_ranges[0] is not None or servo_ranges[1] is not None):
            self.draw_servo(*servo_ranges)
        # the servo torque limit (optional cfg.control.torque_limit / cfg.domain_rand.torque_limit_range; no reference line): set once,
        # here, before the first reset()
        if "torque_limit" in pools:
            pass
        elif torque_range is not None:
            self.draw_torque_limit(torque_range)
        elif torque_limit is not None and np.isfinite(torque_limit).any():
            self.set_torque_limit(torque_limit)
        for kind, values in pools.items():
            self.set_reset_pool(kind, **values)
        # the external wrench on the base (optional cfg.domain_rand; no reference line): the schedule starts at step 0
        self.wrench_interval = 0
        if wrench_sched is not None:
            self.set_wrench_schedule(*wrench_sched)
        # the sensor model - observation latency and bias (optional cfg.domain_rand; no reference line): drawn once, here
        if any(r is not None for r in sensor_ranges):
            self.draw_sensor_model(*sensor_ranges)
        # randomised reset states (optional cfg.domain_rand; no reference line): on before the first reset(), whose reset_idx(all) is
        # draw 0 of every env
        if reset_ranges is not None:
            self.set_reset_noise(reset_ranges)
        # state log of env 0 (reference :261-272; reader open_custom_play.py:50-66)
        self.state_log = None
        self._rec_env = 0
        self._fixed_cmd = None
        self._play_step = 0
        if cfg.viewer.record_states:
            self.state_log = StateLog(log_dir, self.dt)
            self._ck(L.nm_set_state_record(h, 0))

    @property
    def recorded_states(self):
        """Upstream's self.recorded_states (:261-272): what has been logged since the last dump."""
        return self.state_log.records if self.state_log is not None else []

    def set_state_record(self, env_index):
        """Which env the state log follows (nm_set_state_record; upstream logs data[0], :267). Needs cfg.viewer.record_states."""
        if self.state_log is None:
            raise ValueError("set_state_record: cfg.viewer.record_states is off")
        i = int(env_index)
        if not 0 <= i < self.num_envs:
            raise ValueError("set_state_record: env index out of range")
        self._ck(self._L.nm_set_state_record(self._h, i))
        self._rec_env = i

    def _noise_scale_vec(self, cfg):
        ns, lvl, osc = cfg.noise.noise_scales, cfg.noise.noise_level, self.obs_scales
        v = np.zeros(self.num_obs)
        v[:3] = ns.lin_vel * lvl * osc.lin_vel
        v[3:6] = ns.ang_vel * lvl * osc.ang_vel
        v[6:9] = ns.gravity * lvl
        layout = getattr(cfg.noise, "layout", "reference")
        if layout == "reference":       # the upstream index ranges, kept verbatim (they assume 12 dofs)
            v[12:24] = ns.dof_pos * lvl * osc.dof_pos
            v[24:36] = ns.dof_vel * lvl * osc.dof_vel
        elif layout == "dof18":         # the ranges of this robot's observation (E8: dof_pos 12:30, dof_vel 30:48)
            v[12:30] = ns.dof_pos * lvl * osc.dof_pos
            v[30:48] = ns.dof_vel * lvl * osc.dof_vel
        else:
            raise ValueError("cfg.noise.layout must be 'reference' or 'dof18'")
        return v

    def set_noise_uniforms(self, u=None):
        """RNG-free noise for parity tests: [N,66] uniforms in [0,1) used instead of the generator (None = generator)."""
        u = None if u is None else np.ascontiguousarray(u, np.float64).reshape(self.num_envs, self.num_obs)
        self._ck(self._L.nm_set_noise_uniforms(self._h, None if u is None else u.ctypes.data_as(C.c_void_p)))

    def set_push(self, interval_steps, max_vel_xy, start_step=0):
        """Push perturbations (nm_set_push): every `interval_steps` env steps qvel[:, 0:2] of every env is set to a draw from
        U[-max_vel_xy, max_vel_xy) before the physics of that step, in step(), policy_rollout, policy_play and step_tape alike.
        0 steps = off. The env's push step index restarts at start_step."""
        self._ck(self._L.nm_set_push(self._h, int(interval_steps), float(max_vel_xy), int(start_step)))
        self.push_interval, self.max_push_vel_xy = int(interval_steps), float(max_vel_xy)

    def push_state(self):
        """(interval_steps, max_vel_xy, step) as nm_get_push returns them: what a checkpoint needs to continue the push schedule."""
        iv, mx, st = C.c_int32(0), C.c_double(0), C.c_uint64(0)
        self._ck(self._L.nm_get_push(self._h, C.byref(iv), C.byref(mx), C.byref(st)))
        return iv.value, mx.value, st.value

    def set_reset_noise(self, ranges=None, counts=None):
        """Randomised reset states (nm_set_reset_noise): `ranges` = five (lo, hi) pairs in the order base_height, dof_pos, base_lin_vel,
        base_ang_vel, dof_vel (RESET_NOISE_RANGES), or None = off. While on, every reset of an env - in step(), reset_idx, policy_rollout,
        policy_play and step_tape alike - adds a fresh uniform draw to qpos0's base height and joint angles and sets all 24 velocities
        to draws; the draw is keyed by (seed, global env id, the env's reset count). counts: [num_envs] reset counts to install (a
        checkpoint's), None keeps the env's."""
        r = None
        if ranges is not None:
            r = np.ascontiguousarray(ranges, np.float64)
            if r.size != 10:
                raise ValueError("set_reset_noise: ranges must be five (lo, hi) pairs")
            r = (C.c_double * 10)(*r.reshape(-1))
        k = None
        if counts is not None:
            k = np.ascontiguousarray(counts, np.uint32).reshape(-1)
            if k.size != self.num_envs:
                raise ValueError("set_reset_noise: counts must hold num_envs values")
        self._ck(self._L.nm_set_reset_noise(self._h, None if r is None else C.byref(r), None if k is None else k.ctypes.data_as(C.c_void_p)))

    def reset_noise_state(self):
        """(on, ranges [5, 2], counts [num_envs] uint32) as nm_get_reset_noise returns them: what a checkpoint needs to continue the draws."""
        on, r, k = C.c_int32(0), (C.c_double * 10)(), np.zeros(self.num_envs, np.uint32)
        self._ck(self._L.nm_get_reset_noise(self._h, C.byref(on), C.byref(r), k.ctypes.data_as(C.c_void_p)))
        return bool(on.value), np.array(r[:], np.float64).reshape(5, 2), k

    def _per_env(self, x, dtype, err, device=None):
        """num_envs values, or one scalar for every env, as a contiguous [num_envs] tensor of `dtype` on the env's device (or `device`);
        err: the caller's ValueError text for any other count."""
        return per_row_values(x, self.num_envs, dtype, err, self.device if device is None else device)

    def set_env_params(self, mu=None, p_gain=None, kv=None):
        """Per-env sliding friction, servo stiffness (in place of cfg.control.p_gain) and servo damping (in place of kv = 0.8), honoured by
        step(), step_physics, policy_rollout, policy_play and step_tape alike (nm_set_env_params). Each: a tensor / array of num_envs values, a
        scalar for every env, or None = the default. All three None switch the feature off. The values hold until they are set again (no reset
        resamples them) and are not validated: mu <= 1e-5 or a negative gain is the caller's responsibility."""
        cols = env_param_columns(self.num_envs, self._real, self.device, mu, p_gain, kv, "set_env_params: one value per env (or a scalar)")
        self._rows_keep["envp"] = cols
        p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in cols]
        self._ck(self._L.nm_set_env_params(self._h, p[0], p[1], p[2], self._stream()))

    def env_params(self):
        """{'mu', 'p_gain', 'kv'}: tensors [num_envs] in the env's dtype (nm_get_env_params); the defaults while the feature is off."""
        out = {k: torch.empty(self.num_envs, dtype=self._real, device=self.device) for k in ("mu", "p_gain", "kv")}
        self._ck(self._L.nm_get_env_params(self._h, *[C.c_void_p(out[k].data_ptr()) for k in ("mu", "p_gain", "kv")], self._stream()))
        return out

    def draw_env_params(self, friction_range=None, stiffness_multiplier_range=None, damping_multiplier_range=None):
        """Draw every env's parameters on the device (nm_draw_env_params): mu uniform in friction_range, p_gain = cfg.control.p_gain x a
        multiplier uniform in stiffness_multiplier_range, kv = 0.8 x a multiplier uniform in damping_multiplier_range. None pins that value
        to its default. Keyed by the global env id: shards of one population draw what the whole would."""
        mu0, pg, kv0 = self._envp_default          # (mu, p_gain, kv) the library runs with while the feature is off
        fr = (mu0, mu0) if friction_range is None else tuple(float(x) for x in friction_range)
        st = (1.0, 1.0) if stiffness_multiplier_range is None else tuple(float(x) for x in stiffness_multiplier_range)
        da = (1.0, 1.0) if damping_multiplier_range is None else tuple(float(x) for x in damping_multiplier_range)
        lo = (C.c_double * 3)(fr[0], pg * st[0], kv0 * da[0])
        hi = (C.c_double * 3)(fr[1], pg * st[1], kv0 * da[1])
        self._ck(self._L.nm_draw_env_params(self._h, C.byref(lo), C.byref(hi), self._stream()))

    def set_base_payload(self, dm=None, r=None):
        """Per-env base payload: a point mass dm (kg, may be negative) rigidly attached to the base body at r (m, base body frame). The env
        then behaves as if mjmodel.xml had been recompiled with that mass added to base_link - base mass, COM and inertia, total mass,
        the colliding bodies' invweight0 and the solver's scale all follow (model/payload.py derives the rows on the host;
        nm_set_body_params) - in step(), step_physics, policy_rollout, policy_play and step_tape alike. dm: num_envs values or a scalar;
        r: [num_envs, 3], one [3] for every env, or None = the base origin. dm None switches the feature off. The payload holds until
        it is set again (no reset touches it). ValueError: a non-finite value, a base mass <= 0, an inertia that is not positive definite
        or violates the triangle inequality (what MuJoCo's compiler refuses)."""
        if dm is None:
            self._payload = self._rows_keep["body"] = None
            self._ck(self._L.nm_set_body_params(self._h, None, self._stream()))
            return
        dm, r = payload_values(self.num_envs, dm, r, "set_base_payload: one dm per env (or a scalar) and one r[3] per env (or one for all)")
        rows = payload_body_rows(dm, r)
        t = torch.from_numpy(rows).to(dtype=self._real).to(self.device).contiguous()
        self._ck(self._L.nm_set_body_params(self._h, C.c_void_p(t.data_ptr()), self._stream()))
        self._rows_keep["body"] = t
        self._payload = (dm.copy(), r.copy())

    def base_payload(self):
        """{'dm': [num_envs], 'r': [num_envs, 3]} (float64 numpy, what was set: zeros while the feature is off) and 'rows': the
        [num_envs, 20] body rows the kernels read, a tensor in the env's dtype (nm_get_body_params; the model's own row while off)."""
        rows = torch.empty(self.num_envs, 20, dtype=self._real, device=self.device)
        self._ck(self._L.nm_get_body_params(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        dm, r = self._payload if self._payload is not None else (np.zeros(self.num_envs), np.zeros((self.num_envs, 3)))
        return {"dm": dm.copy(), "r": r.copy(), "rows": rows}

    def draw_base_payload(self, mass_range=None, com_range=None):
        """Draw every env's payload on the device (nm_draw_payload: dm uniform in mass_range kg, each of r's components uniform in
        com_range m; None pins that part to 0), derive the rows on the host and set them. Keyed by the global env id: shards of one
        population draw what the whole would. Returns what base_payload() then reports."""
        ma = (0.0, 0.0) if mass_range is None else tuple(float(x) for x in mass_range)
        co = (0.0, 0.0) if com_range is None else tuple(float(x) for x in com_range)
        lo, hi = (C.c_double * 4)(ma[0], co[0], co[0], co[0]), (C.c_double * 4)(ma[1], co[1], co[1], co[1])
        out = torch.empty(self.num_envs, 4, dtype=self._real, device=self.device)
        self._ck(self._L.nm_draw_payload(self._h, C.byref(lo), C.byref(hi), C.c_void_p(out.data_ptr()), self._stream()))
        d = out.to(torch.float64).cpu().numpy()
        self.set_base_payload(d[:, 0], d[:, 1:])
        return self.base_payload()

    ACTION_HISTORY = 3       # past actions an env keeps (nm_core.h kLatH): the longest delay is this many env steps

    def set_action_latency(self, substeps=None):
        """Per-env actuation latency: env e's servo targets lag the policy's actions by substeps[e] physics substeps, 0 <= d <=
        ACTION_HISTORY x decimation (nm_set_action_latency; include/nightmare_hip.h states the semantics). With k = d // decimation and r =
        d % decimation, substep s of step t aims at a_{t-k-1} while s < r and at a_{t-k} afterwards. Observations, rewards, the actions
        buffer and the logs keep a_t: the policy meets latency through the physics alone. Honoured by step(), policy_rollout,
        policy_play and step_tape alike; step_physics ignores it. substeps: num_envs integers, one integer for every env, or None =
        off. The delays hold until they are set again; no reset touches them or the action history."""
        if substeps is None:
            self._rows_keep["lat"] = None
            self._ck(self._L.nm_set_action_latency(self._h, None, self._stream()))
            return
        t = latency_values(self.num_envs, self.device, substeps, "set_action_latency")
        self._ck(self._L.nm_set_action_latency(self._h, C.c_void_p(t.data_ptr()), self._stream()))
        self._rows_keep["lat"] = t

    def action_latency(self):
        """The delays, an int32 tensor [num_envs] in physics substeps (nm_get_action_latency); zeros while the feature is off."""
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._ck(self._L.nm_get_action_latency(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def draw_action_latency(self, lo, hi):
        """Draw every env's delay on the device, uniform on the integers [lo, hi] (nm_draw_action_latency), and switch the feature on.
        Keyed by the global env id: shards of one population draw what the whole would. Returns what action_latency() then reports."""
        if int(lo) != lo or int(hi) != hi:
            raise ValueError("draw_action_latency: whole substeps")
        self._ck(self._L.nm_draw_action_latency(self._h, int(lo), int(hi), self._stream()))
        return self.action_latency()

    def action_history(self):
        """float32 tensor [num_envs, ACTION_HISTORY, 18]: row j is a_{t-1-j}, the scaled and clipped action of j + 1 steps ago
        (nm_get_action_history). Zero at construction; it follows the steps taken while latency is on. reset_idx() leaves it alone;
        reset() is reset_idx() and one step under zero actions, which shifts it like any other step."""
        out = torch.empty(self.num_envs, self.ACTION_HISTORY, 18, dtype=torch.float32, device=self.device)
        self._ck(self._L.nm_get_action_history(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_action_history(self, h):
        """Overwrite the action history ([num_envs, ACTION_HISTORY, 18], the order of action_history()): checkpoints and tests."""
        t = torch.as_tensor(h, dtype=torch.float32).to(self.device).contiguous()
        if tuple(t.shape) != (self.num_envs, self.ACTION_HISTORY, 18):
            raise ValueError("set_action_history: [num_envs, 3, 18]")
        self._ck(self._L.nm_set_action_history(self._h, C.c_void_p(t.data_ptr()), self._stream()))
        self._rows_keep["hist"] = t

    def _vec3(self, v, err):
        """[num_envs, 3] float64 numpy from one [3] for every env or a [num_envs, 3] array / tensor."""
        return vec3_rows(v, self.num_envs, err)

    def set_gravity(self, g=None, gravity_vec=None):
        """Per-env gravity vectors (nm_set_gravity; include/nightmare_hip.h states the semantics). g: the gravity the physics sees, m/s^2
        in the frame of the floor - for an infinite plane a floor inclined by theta is a level floor under g = 9.81 (sin theta cos phi,
        sin theta sin phi, -cos theta) - [num_envs, 3], one [3] for every env, or None = off. gravity_vec: what the env layer rotates into
        the body frame (observation slots 6..8, the orientation reward, the 60 degree termination); None = equal to g, an IMU's view;
        pass upstream's (0, 0, -9.81) to keep its env layer line for line. Honoured by step(), step_physics, policy_rollout, policy_play
        and step_tape alike. The vectors hold until they are set again; no reset touches them. The attribute `gravity_vec` stays
        upstream's constant. ValueError: a wrong shape; the library refuses non-finite values and a zero gravity_vec."""
        if g is None:
            if gravity_vec is not None:
                raise ValueError("set_gravity: gravity_vec needs g")
            self._rows_keep["grav"] = None
            self._ck(self._L.nm_set_gravity(self._h, None, self._stream()))
            return
        rows = gravity_rows(self.num_envs, g, gravity_vec, "set_gravity: one [3] for every env or [num_envs, 3]")
        t = torch.from_numpy(rows).to(dtype=self._real).to(self.device).contiguous()
        self._ck(self._L.nm_set_gravity(self._h, C.c_void_p(t.data_ptr()), self._stream()))
        self._rows_keep["grav"] = t

    def gravity(self):
        """{'g', 'gravity_vec'}: [num_envs, 3] tensors in the env's dtype (nm_get_gravity); (0, 0, -9.81) twice while the feature is off."""
        rows = torch.empty(self.num_envs, 8, dtype=self._real, device=self.device)
        self._ck(self._L.nm_get_gravity(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        return {"g": rows[:, 0:3].clone(), "gravity_vec": rows[:, 4:7].clone()}

    def draw_gravity(self, offset_range=None, tilt_range=None, observed=True):
        """Draw every env's gravity on the device (nm_draw_gravity: three offsets uniform in offset_range m/s^2, a tilt theta uniform in
        tilt_range rad and, whenever a tilt range is given, an azimuth phi uniform in [0, 2 pi); None pins that part to 0), derive
        g = 9.81 (sin theta cos phi, sin theta sin phi, -cos theta) + offset on the host in float64 and set the rows. observed: the env
        layer sees g (True) or keeps upstream's (0, 0, -9.81). Keyed by the global env id: shards of one population draw what the whole
        would. Returns what gravity() then reports."""
        of = (0.0, 0.0) if offset_range is None else tuple(float(x) for x in offset_range)
        ti = (0.0, 0.0) if tilt_range is None else tuple(float(x) for x in tilt_range)
        if not (0.0 <= ti[0] <= ti[1] < np.pi / 2):
            raise ValueError("draw_gravity: tilt_range must be (lo, hi) rad with 0 <= lo <= hi < pi/2")
        az = 0.0 if tilt_range is None else 2.0 * np.pi
        lo, hi = (C.c_double * 5)(of[0], of[0], of[0], ti[0], 0.0), (C.c_double * 5)(of[1], of[1], of[1], ti[1], az)
        out = torch.empty(self.num_envs, 5, dtype=self._real, device=self.device)
        self._ck(self._L.nm_draw_gravity(self._h, C.byref(lo), C.byref(hi), C.c_void_p(out.data_ptr()), self._stream()))
        d = out.to(torch.float64).cpu().numpy()
        g = gravity_from_draw(d[:, 0:3], d[:, 3], d[:, 4])
        self.set_gravity(g, None if observed else np.array([0.0, 0.0, -GRAVITY]))
        return self.gravity()

    def set_servo(self, rate_limit=None, d_gain=None):
        """The servo target model (nm_set_servo; include/nightmare_hip.h states the semantics; reference envs/nightmare_v3_env.py:97,187-188
        and envs/nightmare_v3_config.py:37-38, commented out upstream). rate_limit: the most an env's servo target may move per control
        step, rad, > 0, inf = no limit; d_gain: the damping on the joint velocity buffer, >= 0. Each: num_envs values, a scalar for every
        env, or None = its default (inf, 0). Both None switch the feature off. The observation, the rewards, the actions buffer and the
        logs keep a_t: the policy meets the servo through the physics alone. Honoured by step(), policy_rollout, policy_play and
        step_tape alike; step_physics ignores it. The rows hold until they are set again; no reset touches them, nor the limited targets
        (servo_state()). The library refuses a rate that is not > 0 and a d_gain that is not finite and >= 0."""
        if rate_limit is None and d_gain is None:
            self._rows_keep["servo"] = None
            self._ck(self._L.nm_set_servo(self._h, None, self._stream()))
            return
        rows = servo_rows(self.num_envs, self._real, self.device, rate_limit, d_gain, "set_servo: one value per env (or a scalar)")
        self._ck(self._L.nm_set_servo(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        self._rows_keep["servo"] = rows

    def servo(self):
        """{'rate_limit', 'd_gain'}: [num_envs] tensors in the env's dtype (nm_get_servo); (inf, 0) while the feature is off."""
        rows = torch.empty(self.num_envs, 4, dtype=self._real, device=self.device)
        self._ck(self._L.nm_get_servo(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        return {"rate_limit": rows[:, 0].clone(), "d_gain": rows[:, 1].clone()}

    def draw_servo(self, rate_range=None, d_gain_range=None):
        """Draw every env's servo row on the device (nm_draw_servo: rate uniform in rate_range, rad per control step, 0 < lo <= hi finite;
        d_gain uniform in d_gain_range, 0 <= lo <= hi finite) and switch the feature on. None pins that column to its default (no limit /
        no damping). Keyed by the global env id: shards of one population draw what the whole would. Returns what servo() then reports."""
        rr = None if rate_range is None else tuple(float(x) for x in rate_range)
        dg = (0.0, 0.0) if d_gain_range is None else tuple(float(x) for x in d_gain_range)
        lo, hi = (C.c_double * 2)(1.0 if rr is None else rr[0], dg[0]), (C.c_double * 2)(1.0 if rr is None else rr[1], dg[1])
        self._ck(self._L.nm_draw_servo(self._h, C.byref(lo), C.byref(hi), self._stream()))
        if rr is None:      # the draw takes finite bounds: "no limit" goes in as a column of its own
            self.set_servo(None, self.servo()["d_gain"])
        return self.servo()

    def set_torque_limit(self, limit=None):
        """The servo torque limit (nm_set_torque_limit; include/nightmare_hip.h states the semantics: MuJoCo's actuator forcerange - the
        clamp of mj_fwdActuation and the saturated joints left out of implicitfast's velocity derivative). limit: N m, > 0, inf = no
        limit; a scalar (every joint of every env), 3 values (coxa, femur, tibia of every env), [num_envs] (one value per env) or
        [num_envs, 3]. None switches the feature off. It is physics: step(), step_physics, policy_rollout, policy_play and step_tape
        honour it alike; no observation, reward or log field changes. The rows hold until they are set again; no reset touches them.
        The library refuses a limit that is not > 0."""
        if limit is None:
            self._rows_keep["torque"] = None
            self._ck(self._L.nm_set_torque_limit(self._h, None, self._stream()))
            return
        rows = torque_rows(self.num_envs, self._real, self.device, limit, "set_torque_limit: a scalar, 3 values, [num_envs] or [num_envs, 3]")
        self._ck(self._L.nm_set_torque_limit(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        self._rows_keep["torque"] = rows

    def torque_limit(self):
        """[num_envs, 3] in the env's dtype: every env's (coxa, femur, tibia) limit (nm_get_torque_limit); inf while the feature is off."""
        rows = torch.empty(self.num_envs, 4, dtype=self._real, device=self.device)
        self._ck(self._L.nm_get_torque_limit(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        return rows[:, :3].clone()

    def draw_torque_limit(self, limit_range):
        """Draw every env's three limits on the device (nm_draw_torque_limit: three independent uniform draws per env) and switch the
        feature on. limit_range: (lo, hi) for all three joint types, or [3, 2]; finite, 0 < lo <= hi. Keyed by the global env id: shards of
        one population draw what the whole would. Returns what torque_limit() then reports."""
        a = np.asarray(limit_range, np.float64)
        if a.shape == (2,):
            a = np.tile(a, (3, 1))
        if a.shape != (3, 2):
            raise ValueError("draw_torque_limit: (lo, hi) or [3, 2]")
        lo, hi = (C.c_double * 3)(*a[:, 0]), (C.c_double * 3)(*a[:, 1])
        self._ck(self._L.nm_draw_torque_limit(self._h, C.byref(lo), C.byref(hi), self._stream()))
        return self.torque_limit()

    def set_base_wrench(self, force=None, torque=None):
        """A constant external wrench on the base body (nm_set_base_wrench; include/nightmare_hip.h states the semantics: MuJoCo's
        xfrc_applied on the base). force (N) and torque (N m) are in the world frame, the force applied at the base body's centre of mass;
        each is None (zero), 3 values (every env) or [num_envs, 3]. Both None switches the feature off (and ends a schedule). It is
        physics: step(), step_physics, policy_rollout, policy_play and step_tape honour it alike; no observation, reward or log field
        changes. The rows hold until they are set again; no reset touches them. The library refuses non-finite values, and rows while
        a schedule is on."""
        if force is None and torque is None:
            self._rows_keep["wrench"] = None
            self._ck(self._L.nm_set_base_wrench(self._h, None, self._stream()))
            self.wrench_interval = 0
            return
        n = self.num_envs
        rows = torch.zeros(n, 8, dtype=self._real, device=self.device)
        for col, v in ((0, force), (4, torque)):
            if v is None:
                continue
            t = torch.as_tensor(v, dtype=self._real).detach().to(self.device)
            if t.dim() == 1 and t.numel() == 3:
                t = t.expand(n, 3)
            elif tuple(t.shape) != (n, 3):
                raise ValueError("set_base_wrench: force and torque are 3 values or [num_envs, 3]")
            rows[:, col:col + 3] = t
        self._ck(self._L.nm_set_base_wrench(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        self._rows_keep["wrench"] = rows

    def base_wrench(self):
        """{"force": [num_envs, 3], "torque": [num_envs, 3]} in the env's dtype: the wrench every env's physics reads at its next step
        (nm_get_base_wrench); zero while the feature is off."""
        rows = torch.empty(self.num_envs, 8, dtype=self._real, device=self.device)
        self._ck(self._L.nm_get_base_wrench(self._h, C.c_void_p(rows.data_ptr()), self._stream()))
        return {"force": rows[:, 0:3].clone(), "torque": rows[:, 4:7].clone()}

    def set_wrench_schedule(self, interval_steps, duration_steps, max_force, max_torque, start_step=0):
        """Random wrenches on the base over time windows (nm_set_wrench_schedule): from step interval_steps on, every interval_steps env
        steps every env draws a force uniform in [-max_force, max_force) and a torque uniform in [-max_torque, max_torque) per axis, holds
        them for duration_steps steps (1 <= duration_steps <= interval_steps) and then zero until the next window - in step(),
        policy_rollout, policy_play and step_tape alike. max_force (N), max_torque (N m): a scalar gives all three axes. The env's wrench
        step index restarts at start_step, and the rows that hold there are installed: wrench_schedule()'s numbers continue a run exactly.
        interval_steps = 0 switches the schedule off and the rows to zero. Keyed by the global env id: shards of one population draw
        what the whole would."""
        mf = (C.c_double * 3)(*np.broadcast_to(np.asarray(max_force, np.float64), (3,)))
        mt = (C.c_double * 3)(*np.broadcast_to(np.asarray(max_torque, np.float64), (3,)))
        torch.cuda.current_stream(self.device).synchronize()      # the call is synchronous on the device's null stream
        self._ck(self._L.nm_set_wrench_schedule(self._h, int(interval_steps), int(duration_steps), C.byref(mf), C.byref(mt), int(start_step)))
        self.wrench_interval = int(interval_steps)
        self._rows_keep["wrench"] = None

    def wrench_schedule(self):
        """(interval_steps, duration_steps, max_force[3], max_torque[3], step) as nm_get_wrench_schedule returns them: what a checkpoint
        needs to continue the schedule."""
        iv, du, st = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        mf, mt = (C.c_double * 3)(), (C.c_double * 3)()
        self._ck(self._L.nm_get_wrench_schedule(self._h, C.byref(iv), C.byref(du), C.byref(mf), C.byref(mt), C.byref(st)))
        return iv.value, du.value, list(mf), list(mt), st.value

    # ------------------------------------------------------------------ per-env rows re-drawn at reset, from pools
    @staticmethod
    def _pool_len(*vals, row=None):
        """The pool size the values imply: the leading length of the first value with a row dimension (row: the length of ONE row's
        value - 3 for a vector - or None for a scalar per row); 1 where every value is one row's."""
        for v in vals:
            if v is None:
                continue
            a = v if isinstance(v, torch.Tensor) else np.asarray(v)
            nd = a.dim() if isinstance(a, torch.Tensor) else a.ndim
            if nd > (0 if row is None else 1):
                return int(a.shape[0])
        return 1

    def set_reset_pool(self, kind, size=None, **values):
        """Give one kind of per-env rows a POOL that every reset of an env re-draws its row from (nm_set_reset_rows; include/nightmare_hip.h
        states the semantics): a time-out, a termination or reset_idx - in step(), policy_rollout, policy_play and step_tape alike -
        overwrites that env's row with pool row i, i drawn from (seed, global env id, the env's reset-row count). kind: one of
        RESET_POOL_KINDS; values: what the kind's own setter takes - env_params: mu, p_gain, kv; base_payload: dm, r; action_latency:
        substeps; gravity: g, gravity_vec; servo: rate_limit, d_gain; torque_limit: limit - with a leading pool dimension P in place of
        num_envs (1 <= P <= 65536; `size` states P where every value is a single row's, and three torque limits are one row). It
        switches the kind on; the rows the envs hold stay until each env's next reset. No values: the pool is dropped and the rows stay.
        Switching the kind off through its own setter drops the pool too. The library refuses a pool row the kind's setter would refuse."""
        if kind not in RESET_POOL_KINDS:
            raise ValueError(f"set_reset_pool: kind must be one of {RESET_POOL_KINDS}")
        ki = RESET_POOL_KINDS.index(kind)
        if all(v is None for v in values.values()):
            self._rows_keep["pool_" + kind] = None
            self._ck(self._L.nm_set_reset_rows(self._h, ki, None, 0, self._stream()))
            return
        who, real, dev = f"set_reset_pool({kind!r})", self._real, self.device

        def take(*names):
            extra = set(values) - set(names)
            if extra:
                raise ValueError(f"{who}: takes {', '.join(names)}, not {', '.join(sorted(extra))}")
            return [values.get(n) for n in names]

        err = f"{who}: one value per pool row (or one for all)"
        if kind == "env_params":
            v = take("mu", "p_gain", "kv")
            P = self._pool_len(*v) if size is None else int(size)
            rows = env_param_rows(env_param_columns(P, real, dev, *v, err), self._envp_default, P, real, dev)
        elif kind == "base_payload":
            dm, r = take("dm", "r")
            P = (self._pool_len(dm) if self._pool_len(dm) > 1 else self._pool_len(r, row=3)) if size is None else int(size)
            rows = torch.from_numpy(payload_body_rows(*payload_values(P, 0.0 if dm is None else dm, r, err))).to(dtype=real)
        elif kind == "action_latency":
            (d,) = take("substeps")
            P = self._pool_len(d) if size is None else int(size)
            rows = latency_values(P, dev, d, who)
        elif kind == "gravity":
            g, gv = take("g", "gravity_vec")
            if g is None:
                raise ValueError(f"{who}: gravity_vec needs g")
            P = (self._pool_len(g, row=3) if self._pool_len(g, row=3) > 1 else self._pool_len(gv, row=3)) if size is None else int(size)
            rows = torch.from_numpy(gravity_rows(P, g, gv, f"{who}: one [3] for every pool row or [P, 3]")).to(dtype=real)
        elif kind == "servo":
            v = take("rate_limit", "d_gain")
            P = self._pool_len(*v) if size is None else int(size)
            rows = servo_rows(P, real, dev, *v, err)
        else:
            (lim,) = take("limit")
            a = torch.as_tensor(lim)
            P = (1 if a.dim() == 0 or (a.dim() == 1 and a.numel() == 3) else int(a.shape[0])) if size is None else int(size)
            rows = torque_rows(P, real, dev, lim, f"{who}: a scalar, 3 values, [P] or [P, 3]")
        if not 1 <= P <= RESET_POOL_MAX:
            raise ValueError(f"{who}: a pool holds 1..{RESET_POOL_MAX} rows")
        rows = rows.to(dev).contiguous()
        self._ck(self._L.nm_set_reset_rows(self._h, ki, C.c_void_p(rows.data_ptr()), P, self._stream()))
        self._rows_keep["pool_" + kind] = rows

    def reset_pool(self, kind):
        """(rows, P) of the kind's pool - rows a [P, width] tensor in the env's dtype as the kernels read it (nm_get_reset_rows; [P] int32
        for action_latency) - or None while the kind has no pool."""
        if kind not in RESET_POOL_KINDS:
            raise ValueError(f"reset_pool: kind must be one of {RESET_POOL_KINDS}")
        ki = RESET_POOL_KINDS.index(kind)
        P = C.c_int32(0)
        self._ck(self._L.nm_get_reset_rows(self._h, ki, C.byref(P), None, self._stream()))
        if P.value == 0:
            return None
        rows = (torch.empty(P.value, dtype=torch.int32, device=self.device) if kind == "action_latency"
                else torch.empty(P.value, RESET_POOL_WIDTH[ki], dtype=self._real, device=self.device))
        self._ck(self._L.nm_get_reset_rows(self._h, ki, None, C.c_void_p(rows.data_ptr()), self._stream()))
        return rows, P.value

    def reset_row_counts(self):
        """[num_envs] uint32 numpy: how often each env's rows have been re-drawn (nm_get_reset_row_counts); a checkpoint's content."""
        k = np.zeros(self.num_envs, np.uint32)
        self._ck(self._L.nm_get_reset_row_counts(self._h, k.ctypes.data_as(C.c_void_p)))
        return k

    def set_reset_row_counts(self, counts):
        """Install [num_envs] reset-row counts (a checkpoint's): the next reset of env e draws with counts[e]."""
        k = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if k.size != self.num_envs:
            raise ValueError("set_reset_row_counts: counts must hold num_envs values")
        self._ck(self._L.nm_set_reset_row_counts(self._h, k.ctypes.data_as(C.c_void_p)))

    def servo_state(self):
        """[num_envs, 18] float64 numpy: every env's rate-limited servo target L, upstream's limited_actions (nm_get_servo_state), in the
        env's precision. Zero at construction; it follows the steps taken while the servo model is on. reset_idx() leaves it alone;
        reset() is reset_idx() and one step under zero actions, which updates it like any other step."""
        out = np.empty((self.num_envs, 18))
        self._ck(self._L.nm_get_servo_state(self._h, out.ctypes.data))
        return out

    def set_servo_state(self, limited):
        """Overwrite the limited targets ([num_envs, 18]): checkpoints and tests."""
        a = np.ascontiguousarray(limited, np.float64)
        if a.shape != (self.num_envs, 18):
            raise ValueError("set_servo_state: [num_envs, 18]")
        self._ck(self._L.nm_set_servo_state(self._h, a.ctypes.data))

    # ------------------------------------------------------------------ the sensor model (nm_sensor.h; no reference line)
    def set_sensor_model(self, imu_delay=None, joint_delay=None, bias=None):
        """Per-env observation latency and bias (nm_set_sensor; include/nightmare_hip.h states the semantics): columns 0..8 of the
        observation (base velocities, projected gravity) arrive imu_delay[e] whole env steps late, columns 12..47 (dof_pos, dof_vel)
        joint_delay[e] steps late, 0 <= d <= 3, and both carry the constant offset bias[e] ([66] float32, observation units, zero in the
        command and action columns, which are never delayed or biased). What step(), get_observations(), policy_rollout, policy_play and
        step_tape hand out, what the policy inside the launches reads and what the storage keeps is then the sensed row;
        true_observations() is the step's own. imu_delay / joint_delay: num_envs integers, one integer for every env, or None = 0;
        bias: [num_envs, 66], one row [66] for every env, or None = 0. All three None: off. Setting the model clears its history."""
        N, dev = self.num_envs, self.device
        if imu_delay is None and joint_delay is None and bias is None:
            self._rows_keep["sensor"] = None
            self._ck(self._L.nm_set_sensor(self._h, None, None, self._stream()))
            return
        cols = []
        for name, d in (("imu_delay", imu_delay), ("joint_delay", joint_delay)):
            a = np.asarray(0 if d is None else (d.detach().cpu().numpy() if torch.is_tensor(d) else d))
            if a.size not in (1, N) or not np.array_equal(a, np.round(a)):
                raise ValueError(f"set_sensor_model: {name} must be one whole number or num_envs of them")
            cols.append(np.broadcast_to(a.reshape(-1), (N,)).astype(np.int32))
        dl = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=1))).to(dev)
        bt = None
        if bias is not None:
            b = torch.as_tensor(bias, dtype=torch.float32)
            if tuple(b.shape) not in ((self.num_obs,), (N, self.num_obs)):
                raise ValueError(f"set_sensor_model: bias must be [{self.num_obs}] or [{N}, {self.num_obs}]")
            bt = b.expand(N, self.num_obs).to(dev).contiguous()
        self._ck(self._L.nm_set_sensor(self._h, C.c_void_p(dl.data_ptr()), None if bt is None else C.c_void_p(bt.data_ptr()), self._stream()))
        self._rows_keep["sensor"] = (dl, bt)

    def sensor_model(self):
        """{'on': bool, 'imu_delay': int32 [num_envs], 'joint_delay': int32 [num_envs], 'bias': float32 [num_envs, 66]} on the env's device
        (nm_get_sensor); zeros while the model is off."""
        on = C.c_int32(0)
        dl = torch.empty((self.num_envs, 2), dtype=torch.int32, device=self.device)
        b = torch.empty((self.num_envs, self.num_obs), dtype=torch.float32, device=self.device)
        self._ck(self._L.nm_get_sensor(self._h, C.byref(on), C.c_void_p(dl.data_ptr()), C.c_void_p(b.data_ptr()), self._stream()))
        return {"on": bool(on.value), "imu_delay": dl[:, 0].contiguous(), "joint_delay": dl[:, 1].contiguous(), "bias": b}

    def draw_sensor_model(self, imu_latency_range=None, joint_latency_range=None, bias_max=None):
        """Draw every env's delays and bias on the device (nm_draw_sensor) and switch the model on: each delay uniform on the integers of
        its (lo, hi) range (None: 0), each bias column uniform in +-bias_max[kind] (a dict of any of lin_vel, ang_vel, gravity, dof_pos,
        dof_vel, in observation units; a missing kind or None: 0). Keyed by the global env id: shards of one population draw what the whole
        would. Returns what sensor_model() then reports."""
        lo, hi = (C.c_int32 * 2)(), (C.c_int32 * 2)()
        for g, (name, r) in enumerate((("imu_latency_range", imu_latency_range), ("joint_latency_range", joint_latency_range))):
            a, b = (0, 0) if r is None else r
            if int(a) != a or int(b) != b:
                raise ValueError(f"draw_sensor_model: {name}: whole env steps")
            lo[g], hi[g] = int(a), int(b)
        bm = dict(bias_max or {})
        unknown = sorted(set(bm) - set(SENSOR_BIAS_KINDS))
        if unknown:
            raise ValueError(f"draw_sensor_model: unknown bias kinds {unknown} (known: {list(SENSOR_BIAS_KINDS)})")
        mx = (C.c_double * 5)(*[float(bm.get(k, 0.0)) for k in SENSOR_BIAS_KINDS])
        self._ck(self._L.nm_draw_sensor(self._h, C.byref(lo), C.byref(hi), C.byref(mx), self._stream()))
        return self.sensor_model()

    def sensor_state(self):
        """(ring float32 [num_envs, 4, 66], count uint32 [num_envs]) numpy: every env's last true observations - slot n % 4 takes the push
        of an env whose count is n - and the number pushed since the history was last cleared (nm_get_sensor_state). A checkpoint's content."""
        ring = np.zeros((self.num_envs, SENSOR_SLOTS, self.num_obs), np.float32)
        count = np.zeros(self.num_envs, np.uint32)
        self._ck(self._L.nm_get_sensor_state(self._h, ring.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p)))
        return ring, count

    def set_sensor_state(self, ring, count=None):
        """Overwrite the history (what sensor_state() returns, as two arguments or as its tuple): checkpoints and tests."""
        if count is None:
            ring, count = ring
        r, k = np.ascontiguousarray(ring, np.float32), np.ascontiguousarray(count, np.uint32).reshape(-1)
        if r.shape != (self.num_envs, SENSOR_SLOTS, self.num_obs) or k.size != self.num_envs:
            raise ValueError(f"set_sensor_state: ring [{self.num_envs}, {SENSOR_SLOTS}, {self.num_obs}] and count [{self.num_envs}]")
        self._ck(self._L.nm_set_sensor_state(self._h, r.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)))

    def true_observations(self):
        """float32 [num_envs, 66], a fresh tensor: the observation the last step itself produced, before the sensor model
        (nm_get_true_obs); while the model is off, a copy of get_observations()."""
        if not self.sensor_model()["on"]:
            return self.obs_buf.clone()
        out = torch.empty((self.num_envs, self.num_obs), dtype=torch.float32, device=self.device)
        self._ck(self._L.nm_get_true_obs(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def _record_state(self):
        # reference :261-272: when env 0 resets, dump what was logged so far, then log (time, qpos, qvel, act) of env 0
        # as it is after the physics and before reset_idx. This model has no actuator state: act is empty.
        # The order, the clock and the files are StateLog's.
        qpos, qvel, nbad = np.empty(25), np.empty(24), C.c_int32(0)
        self._ck(self._L.nm_get_state_record(self._h, qpos.ctypes.data_as(C.c_void_p), qvel.ctypes.data_as(C.c_void_p), C.byref(nbad)))
        self.state_log.add(qpos, qvel, nbad.value, bool(self.reset_buf[self._rec_env].item()))

    def _record_launch(self, K, dones=None):
        """The K log rows of the K-step launch just enqueued -> StateLog. dones: the logged env's K reset flags as a device tensor
        (policy_rollout: a column of the storage), None: kept by the launch itself (nm_play). One host synchronisation."""
        if dones is not None:
            d = dones.reshape(-1).to("cpu").numpy()          # waits for the launch
        rows = np.empty((K, _LOG_ROW))
        self._ck(self._L.nm_get_state_log(self._h, 0, K, rows.ctypes.data_as(C.c_void_p)))
        if dones is None:
            d = np.empty(K, np.uint8)
            self._ck(self._L.nm_get_state_log_dones(self._h, 0, K, d.ctypes.data_as(C.c_void_p)))
        self.state_log.add_rows(rows, d)

    def _ck(self, rc):
        _lib.check(rc, self._L)

    # ------------------------------------------------------------------ reference surface
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _eplen(self):
        b = self.episode_length_buf
        if b.device != self.device or b.dtype != torch.int64 or not b.is_contiguous():
            b = b.to(device=self.device, dtype=torch.int64).contiguous()
            self.episode_length_buf = b
        return b

    def _fill_extras(self):
        # reference :363-371: one 0-d float32 tensor per reward + time_outs; views of buffers the kernel refreshes
        # keys = the reward table (non-zero scales), in its order - what upstream's episode_sums holds (:140, :363-367)
        self.extras["episode"] = {"rew_" + n: self._ep_stats[self._stat_names.index(n)] for n in self.reward_scales}
        if self.cfg.env.send_timeouts:
            self.extras["time_outs"] = self.time_out_buf

    def step(self, actions):
        a = actions
        if a.device != self.device or a.dtype != torch.float32:
            a = a.to(device=self.device, dtype=torch.float32)
        if a.dim() != 2 or a.shape[0] != self.num_envs or a.shape[1] < 18:
            raise ValueError(f"actions must be [{self.num_envs}, 18], got {tuple(a.shape)}")
        if a.shape[1] != 18 or not a.is_contiguous():
            a = a[:, :18].contiguous()
        ep = self._eplen()
        self._obs_idx ^= 1
        self.obs_buf = self._obs_pair[self._obs_idx]
        if self.time_out_buf is not self._to_bound:
            # the caller replaced extras' time-out tensor: a caching allocator may hand out the old address again, which the kernel's
            # address check cannot tell from "the buffer I refreshed last" - make the next refresh a full rewrite
            self._ck(self._L.nm_invalidate_time_outs(self._h, self._stream()))
            self._to_bound = self.time_out_buf
            if "time_outs" in self.extras:
                self.extras["time_outs"] = self.time_out_buf
        self._ck(self._L.nm_step(self._h, a.data_ptr(), ep.data_ptr(), self.obs_buf.data_ptr(), self.rew_buf.data_ptr(),
                                   self.reset_buf.data_ptr(), self.time_out_buf.data_ptr(), self._ep_stats.data_ptr(), self._stream()))
        self._last_actions = a  # keep the input alive until the kernel has read it
        self.common_step_counter += 1
        if self.state_log is not None:
            self._record_state()
        if "episode" not in self.extras:
            self._fill_extras()
        if self.privileged_obs_has_obs_prefix:
            # behind the step's own launches: the row shows the per-env rows and the state as they left them (nm_privileged_obs)
            self.privileged_obs_buf = self._priv_pair[self._obs_idx]
            self._ck(self._L.nm_privileged_obs(self._h, self.obs_buf.data_ptr(), self.privileged_obs_buf.data_ptr(), self._stream()))
        return self.obs_buf, self.privileged_obs_buf, self.rew_buf, self.reset_buf, self.extras

    # ------------------------------------------------------------------ K steps per launch with the policy in the env's wave
    def _kstep_launch_args(self, a, obs_field, params_flat, seed, iter_dev, ep):
        """What policy_rollout and policy_play fill alike in their argument struct `a`: a stale time-out tensor is invalidated, the
        observation pair is swapped (a.obs0_dev = the current observation, a.<obs_field> = the buffer the launch leaves its last one in)
        and the env's own buffers and ep = (ep_idx, ep_acc) or None are bound. Returns (ep_idx, ep_acc)."""
        if self.time_out_buf is not self._to_bound:
            self._ck(self._L.nm_invalidate_time_outs(self._h, self._stream()))
            self._to_bound = self.time_out_buf
        a.params_flat_dev, a.seed, a.iter_dev = params_flat.data_ptr(), int(seed), iter_dev.data_ptr()
        a.obs0_dev = self.obs_buf.data_ptr()
        self._obs_idx ^= 1
        self.obs_buf = self._obs_pair[self._obs_idx]           # the tensor handed out before the launch stays what it was
        setattr(a, obs_field, self.obs_buf.data_ptr())
        a.episode_length_dev = self._eplen().data_ptr()
        a.rew_dev, a.done_dev = self.rew_buf.data_ptr(), self.reset_buf.data_ptr()
        a.time_outs_dev, a.ep_stats_dev = self.time_out_buf.data_ptr(), self._ep_stats.data_ptr()
        ep_idx, ep_acc = ep if ep is not None else (None, None)
        a.ep_idx_dev, a.n_ep, a.ep_acc_dev = (ep_idx.data_ptr(), int(ep_idx.numel()), ep_acc.data_ptr()) if ep_idx is not None else (None, 0, None)
        return ep_idx, ep_acc

    def policy_rollout(self, steps, params_flat, seed, iter_dev, storage, gamma, cur_ret, cur_len, fin, ep=None, last_values=None, activation="elu"):
        """`steps` iterations of rsl_rl's collection loop `act -> env.step -> process_env_step` (OnPolicyRunner.learn; reference
        train.py:54) as ONE launch (nm_rollout): starts from the current observation, files every transition into `storage` (a
        RolloutStorage with `steps` rows: observations, actions, values, log-probabilities, mu, sigma, rewards incl. the time-out bootstrap,
        dones), updates the runner's bookkeeping tensors (cur_ret / cur_len [N], fin [3], and ep = (ep_idx int32, ep_acc) for the running
        sum of extras['episode']) and leaves the env as `steps` calls of step() would: obs_buf / rew_buf / reset_buf / extras of the last step.
        params_flat: the flat parameter vector of FusedUpdate (actor W0 b0 ..., critic ..., std). last_values ([N] float32 on the device,
        optional) receives the critic's value of the last observation - what PPO.compute_returns evaluates next. activation: the networks'
        hidden activation (a name of _lib.ACTIVATIONS, as ActorCritic takes it). With cfg.viewer.record_states the launch keeps the state log's
        K rows on the device and they are read - one host synchronisation - after it has been enqueued.
        A storage with privileged rows of this env's width (89, observations 66) on an env with cfg.env.privileged_obs takes the asymmetric
        launch (nm_rollout_priv): params_flat is then the 66 / 89 networks' vector, the first act reads the env's current privileged row,
        every act's row is filed in storage.privileged_observations, and get_privileged_observations() is afterwards the row of the last
        step, double-buffered as step() does it."""
        T = int(steps)
        priv = self._storage_takes_priv_rows(storage)
        if storage.num_transitions_per_env < T or storage.num_envs != self.num_envs or (storage.privileged_observations is not None and not priv):
            raise ValueError("policy_rollout: storage must hold `steps` rows of this env's transitions (no privileged observations)")
        a = _lib.NmRolloutArgs()
        a.steps = T
        ep_idx, ep_acc = self._kstep_launch_args(a, "obs_final_dev", params_flat, seed, iter_dev, ep)
        a.bootstrap_time_outs = 1 if self.cfg.env.send_timeouts else 0
        a.s_obs, a.s_actions, a.s_logp, a.s_values = (storage.observations.data_ptr(), storage.actions.data_ptr(), storage.actions_log_prob.data_ptr(),
                                                       storage.values.data_ptr())
        a.s_mu, a.s_sigma, a.s_rewards, a.s_dones = storage.mu.data_ptr(), storage.sigma.data_ptr(), storage.rewards.data_ptr(), storage.dones.data_ptr()
        a.gamma = float(gamma)
        a.cur_ret, a.cur_len, a.fin3 = cur_ret.data_ptr(), cur_len.data_ptr(), fin.data_ptr()
        a.last_values_dev = last_values.data_ptr() if last_values is not None else None
        if priv:
            pa = _lib.NmRolloutPrivArgs()
            pa.priv0_dev = self.privileged_obs_buf.data_ptr()
            self.privileged_obs_buf = self._priv_pair[self._obs_idx]      # (the index _kstep_launch_args has just swapped)
            pa.priv_final_dev, pa.s_priv = self.privileged_obs_buf.data_ptr(), storage.privileged_observations.data_ptr()
            self._ck(self._L.nm_rollout_priv(self._h, C.byref(a), C.byref(pa), _lib.activation_code(activation), self._stream()))
        else:
            self._ck(self._L.nm_rollout_ex(self._h, C.byref(a), _lib.activation_code(activation), self._stream()))
        self._keep_rollout = (params_flat, iter_dev, storage, cur_ret, cur_len, fin, ep_idx, ep_acc, last_values)
        self.common_step_counter += T
        storage.step = T
        if "episode" not in self.extras:
            self._fill_extras()
        if self.state_log is not None:
            self._record_launch(T, storage.dones[:T, self._rec_env])
        return self.obs_buf

    def policy_play(self, steps, params_flat, *, deterministic=False, seed=0, iter_dev=None, activation="elu", stats=None, step0=None):
        """`steps` iterations of the reference's play loop (play.py:118-132: `actions = nn.act(obs)`, scale / clip, servo command, mj_step x
        decimation) in launches of up to 4096 steps each (nm_play), nothing collected for PPO. Starts from the current observation; returns
        the last one and leaves obs_buf / rew_buf / reset_buf / extras / episode_length_buf / common_step_counter as `steps` calls of step()
        would. `steps` may exceed the episode length.
        params_flat: the flat `actor ..., critic ..., std` vector policy_rollout reads (flat_params_from_state_dict builds it from a
        checkpoint). deterministic: the actor's mean (rsl_rl act_inference) instead of upstream's sampled nn.act. Noise keys: (seed,
        iter_dev[0] * 4096 + step, env, action pair) as policy_act's, where step continues over consecutive calls (step0=None) or
        starts at step0. stats (all optional, float32 device tensors owned by the caller): 'cur_ret', 'cur_len' [N] and 'fin' [3] as the
        runner keeps them, 'ret_sum', 'ret_cnt' [N] = per env the sum and the number of the returns of the episodes it finished,
        'ep' = (ep_idx int32, ep_acc) for the running sum of extras['episode']. With cfg.viewer.record_states every launch's log rows are read
        after it has been enqueued (one host synchronisation per launch)."""
        T = int(steps)
        if T < 1:
            raise ValueError("policy_play: steps must be at least 1")
        st = dict(stats or {})
        unknown = set(st) - {"cur_ret", "cur_len", "fin", "ret_sum", "ret_cnt", "ep"}
        if unknown:
            raise ValueError(f"policy_play: unknown stats {sorted(unknown)}")
        N, dev = self.num_envs, self.device
        for k in ("cur_ret", "cur_len", "ret_sum", "ret_cnt", "fin"):
            t = st.get(k)
            if t is not None and (t.dtype != torch.float32 or t.numel() != (3 if k == "fin" else N) or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"policy_play: stats[{k!r}] must be a contiguous float32 tensor of {3 if k == 'fin' else N} entries on the env's device")
        if (st.get("cur_ret") is None) != (st.get("cur_len") is None) or (st.get("ret_sum") is None) != (st.get("ret_cnt") is None):
            raise ValueError("policy_play: stats 'cur_ret' / 'cur_len' and 'ret_sum' / 'ret_cnt' come in pairs")
        if iter_dev is None:
            if getattr(self, "_play_iter", None) is None:
                self._play_iter = torch.zeros(1, dtype=torch.int64, device=dev)
            iter_dev = self._play_iter
        if getattr(self, "_play_actions", None) is None:
            self._play_actions = torch.zeros((N, self.num_actions), dtype=torch.float32, device=dev)
        if step0 is not None:
            self._play_step = int(step0)
        ptr = lambda t: None if t is None else t.data_ptr()
        a = _lib.NmPlayArgs()
        a.deterministic, a.actions_dev = int(bool(deterministic)), self._play_actions.data_ptr()
        self._kstep_launch_args(a, "obs_dev", params_flat, seed, iter_dev, st.get("ep"))
        a.cur_ret, a.cur_len, a.fin3, a.ret_sum, a.ret_cnt = (ptr(st.get(k)) for k in ("cur_ret", "cur_len", "fin", "ret_sum", "ret_cnt"))
        self._keep_play = (params_flat, iter_dev, st)
        code = _lib.activation_code(activation)
        done = 0
        while done < T:
            k = min(T - done, 4096)
            a.steps, a.step0 = k, self._play_step
            self._ck(self._L.nm_play(self._h, C.byref(a), code, self._stream()))
            a.obs0_dev = a.obs_dev                            # the next launch goes on from what this one left
            self._play_step += k
            self.common_step_counter += k
            done += k
            if self.state_log is not None:
                self._record_launch(k)
        if "episode" not in self.extras:
            self._fill_extras()
        return self.obs_buf

    # ------------------------------------------------------------------ K steps per launch from an action tape
    def step_tape(self, actions, *, record=None, stats=None):
        """K x step(actions[t]) (reference custom_play.py:66-76 around :145-311; any caller that already has its actions) in launches of up to
        4096 steps each (nm_step_tape): no policy, no sampling, the env's wavefront reads row t of the tape before step t. Returns the last
        observation and leaves obs_buf / rew_buf / reset_buf / extras / episode_length_buf / common_step_counter as the K calls of step()
        would, bit for bit. K may exceed the episode length.
        actions: contiguous float32 [K, num_envs, 18] on the env's device (it must stay alive until the launch has run).
        record (all optional, tensors owned by the caller, contiguous, on the env's device): 'obs' float32 [K,N,66], 'rew' float32 [K,N],
        'done' uint8 [K,N] - what every step returned. stats: as policy_play's. With cfg.viewer.record_states every launch's log rows are
        read after it has been enqueued (one host synchronisation per launch)."""
        N, dev = self.num_envs, self.device
        if not torch.is_tensor(actions) or actions.dim() != 3 or actions.shape[1] != N or actions.shape[2] != self.num_actions:
            raise ValueError(f"step_tape: actions must be a [K, {N}, {self.num_actions}] tensor, got {tuple(getattr(actions, 'shape', ()))}")
        if actions.dtype != torch.float32 or actions.device != dev or not actions.is_contiguous():
            raise ValueError("step_tape: actions must be a contiguous float32 tensor on the env's device")
        T = int(actions.shape[0])
        if T < 1:
            raise ValueError("step_tape: the tape must hold at least 1 step")
        rec = dict(record or {})
        unknown = set(rec) - {"obs", "rew", "done"}
        if unknown:
            raise ValueError(f"step_tape: unknown record {sorted(unknown)}")
        shapes = {"obs": ((T, N, self.num_obs), torch.float32), "rew": ((T, N), torch.float32), "done": ((T, N), torch.uint8)}
        for k, t in rec.items():
            shp, dt = shapes[k]
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"step_tape: record[{k!r}] must be a contiguous {str(dt).split('.')[-1]} tensor of shape {shp} on the env's device")
        st = dict(stats or {})
        unknown = set(st) - {"cur_ret", "cur_len", "fin", "ret_sum", "ret_cnt", "ep"}
        if unknown:
            raise ValueError(f"step_tape: unknown stats {sorted(unknown)}")
        for k in ("cur_ret", "cur_len", "ret_sum", "ret_cnt", "fin"):
            t = st.get(k)
            if t is not None and (t.dtype != torch.float32 or t.numel() != (3 if k == "fin" else N) or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"step_tape: stats[{k!r}] must be a contiguous float32 tensor of {3 if k == 'fin' else N} entries on the env's device")
        if (st.get("cur_ret") is None) != (st.get("cur_len") is None) or (st.get("ret_sum") is None) != (st.get("ret_cnt") is None):
            raise ValueError("step_tape: stats 'cur_ret' / 'cur_len' and 'ret_sum' / 'ret_cnt' come in pairs")
        if self.time_out_buf is not self._to_bound:
            self._ck(self._L.nm_invalidate_time_outs(self._h, self._stream()))
            self._to_bound = self.time_out_buf
        ptr = lambda t: None if t is None else t.data_ptr()
        a = _lib.NmTapeArgs()
        self._obs_idx ^= 1
        self.obs_buf = self._obs_pair[self._obs_idx]           # the tensor handed out before the launch stays what it was
        a.obs_dev = self.obs_buf.data_ptr()
        a.episode_length_dev = self._eplen().data_ptr()
        a.rew_dev, a.done_dev = self.rew_buf.data_ptr(), self.reset_buf.data_ptr()
        a.time_outs_dev, a.ep_stats_dev = self.time_out_buf.data_ptr(), self._ep_stats.data_ptr()
        ep_idx, ep_acc = st["ep"] if st.get("ep") is not None else (None, None)
        a.ep_idx_dev, a.n_ep, a.ep_acc_dev = (ep_idx.data_ptr(), int(ep_idx.numel()), ep_acc.data_ptr()) if ep_idx is not None else (None, 0, None)
        a.cur_ret, a.cur_len, a.fin3, a.ret_sum, a.ret_cnt = (ptr(st.get(k)) for k in ("cur_ret", "cur_len", "fin", "ret_sum", "ret_cnt"))
        self._keep_tape = (actions, rec, st)
        done = 0
        while done < T:
            k = min(T - done, 4096)
            a.steps, a.actions_dev = k, actions[done].data_ptr()
            a.rec_obs_dev, a.rec_rew_dev, a.rec_done_dev = (ptr(rec[n][done]) if rec.get(n) is not None else None for n in ("obs", "rew", "done"))
            self._ck(self._L.nm_step_tape(self._h, C.byref(a), self._stream()))
            self.common_step_counter += k
            done += k
            if self.state_log is not None:
                self._record_launch(k)
        if "episode" not in self.extras:
            self._fill_extras()
        return self.obs_buf

    def joint_target_servo(self, action_rate):
        """The `servo` argument of nikengine.EngineNode.tape for this env: custom_play.py:72's rate limit (`action_rate` rad per step) followed
        by the inverse of step()'s action -> joint target mapping (actions_from_joint_targets, as a multiplication by float32(1 /
        action_scale)), with a zeroed [N,18] float32 `targets` tensor - the rate limiter's memory, updated by every tape."""
        return dict(targets=torch.zeros((self.num_envs, 18), dtype=torch.float32, device=self.device), action_rate=float(action_rate),
                    default_pos=[float(x) for x in self.default_dof_pos[:3]], action_scale=float(self.cfg.control.action_scale))

    def set_fixed_commands(self, cmd):
        """Hold the velocity command (vx, yaw) for ALL envs across the periodic resample (:235) and the resample at a reset (:356):
        the uniforms that map onto it are injected at every resample (nm_set_command_uniforms) and `commands` is written once, now.
        None: back to the env's own resampling (the commands then change at each env's next resample). A command outside
        cfg.commands.ranges (max_lin_vel_x, max_ang_vel) is a ValueError. Upstream's zeroing of small commands still applies: a command
        whose linear part has norm <= 0.02 is held as (0, yaw) (:333, `commands[:, :2] *= norm > 0.02`). The resample computes
        u * 2 * max - max in the env's precision, so the held value is the requested one to one ulp."""
        if cmd is None:
            self._fixed_cmd = None
            self.set_command_uniforms(None)
            return
        vx, yaw = (float(x) for x in cmd)
        mx, ma = float(self.command_ranges.max_lin_vel_x), float(self.command_ranges.max_ang_vel)
        if not (abs(vx) <= mx and abs(yaw) <= ma) or mx <= 0 or ma <= 0:
            raise ValueError(f"set_fixed_commands: ({vx}, {yaw}) is outside the command ranges (|vx| <= {mx}, |yaw| <= {ma})")
        ux, uy = (vx + mx) / (2 * mx), (yaw + ma) / (2 * ma)
        self.set_command_uniforms(np.tile(np.array([ux, uy, ux, uy]), (self.num_envs, 1)))
        keep = 1.0 if abs(vx) > 0.02 else 0.0
        self.set_buffers(commands=np.tile(np.array([vx * keep, 0.0, yaw]), (self.num_envs, 1)))
        self._fixed_cmd = (vx, yaw)

    def _storage_takes_priv_rows(self, storage):
        """Does `storage` ask for the asymmetric wave policy - privileged rows of this env's width next to observation rows, on an env that
        hands such rows out?"""
        p = storage.privileged_observations
        return bool(p is not None and self.privileged_obs_has_obs_prefix and p.shape[-1] == self.num_privileged_obs
                    and storage.observations.shape[-1] == self.num_obs)

    def policy_act(self, params_flat, obs, seed, iter_dev, step, storage, activation="elu"):
        """PPO.act as one launch of the rollout's wave code (nm_rollout_act_ex): the per-step counterpart of policy_rollout. A storage with
        privileged rows (policy_rollout says which) takes nm_rollout_act_priv: `obs` is then the [N, 89] row; the row goes to
        storage.privileged_observations[step], its first 66 columns to storage.observations[step]."""
        s = int(step)
        if storage.privileged_observations is not None:
            if not self._storage_takes_priv_rows(storage) or obs.shape[-1] != self.num_privileged_obs:
                raise ValueError("policy_act: privileged rows need cfg.env.privileged_obs, a storage of this env's widths and the wide row as `obs`")
            self._ck(self._L.nm_rollout_act_priv(self._h, params_flat.data_ptr(), obs.data_ptr(), int(seed), iter_dev.data_ptr(), s, storage.actions[s].data_ptr(),
                                                 storage.actions_log_prob[s].data_ptr(), storage.values[s].data_ptr(), storage.mu[s].data_ptr(),
                                                 storage.sigma[s].data_ptr(), storage.observations[s].data_ptr(), storage.privileged_observations[s].data_ptr(),
                                                 _lib.activation_code(activation), self._stream()))
            return storage.actions[s]
        self._ck(self._L.nm_rollout_act_ex(self._h, params_flat.data_ptr(), obs.data_ptr(), int(seed), iter_dev.data_ptr(), s, storage.actions[s].data_ptr(),
                                           storage.actions_log_prob[s].data_ptr(), storage.values[s].data_ptr(), storage.mu[s].data_ptr(),
                                           storage.sigma[s].data_ptr(), storage.observations[s].data_ptr(), _lib.activation_code(activation), self._stream()))
        return storage.actions[s]

    def actions_from_joint_targets(self, targets):
        """Policy-space actions that make the servo track absolute joint targets (the hook at reference :186):
        step() commands (action_scale*a - default_pos - dof_pos)*p_gain (:152-156,:183-188), so a = (q* + default_pos)/action_scale.
        Targets beyond clip_actions - default_pos saturate, as any action does."""
        d = getattr(self, "_default_t", None)
        if d is None:
            d = self._default_t = torch.as_tensor(self.default_dof_pos, dtype=torch.float32, device=self.device)
        return (targets.to(device=self.device, dtype=torch.float32) + d) / float(self.cfg.control.action_scale)

    def step_physics(self, actions):
        """mj_step x decimation only (no rewards/obs/reset): the 'dynamics+contact kernel' configuration."""
        a = actions.to(device=self.device, dtype=torch.float32)[:, :18].contiguous()
        self._ck(self._L.nm_step_physics(self._h, a.data_ptr(), self._stream()))
        self._last_actions = a

    def reset_idx(self, env_ids):
        if env_ids is None:
            ids, n = None, 0
        else:
            idsa = np.ascontiguousarray(torch.as_tensor(env_ids).detach().cpu().numpy().astype(np.int32))
            if idsa.size == 0:
                return
            ids, n = idsa.ctypes.data_as(C.c_void_p), int(idsa.size)
        ep = self._eplen()
        self._ck(self._L.nm_reset(self._h, ids, n, ep.data_ptr(), self._ep_stats.data_ptr(), self._stream()))
        self._fill_extras()

    def reset(self):
        self.reset_idx(None)
        obs, priv, _, _, _ = self.step(torch.zeros((self.num_envs, self.num_actions), device=self.device))
        return obs, priv

    def get_observations(self):
        return self.obs_buf

    def get_privileged_observations(self):
        """None (the reference, :317-319) unless cfg.env.privileged_obs is on: then the [num_envs, 89] row of the last step() (envs/privileged.py).
        policy_rollout into a storage with privileged rows leaves the row of its last step; policy_play, step_tape and the symmetric
        policy_rollout evaluate no critic outside their launch and do not refresh it."""
        return self.privileged_obs_buf

    def privileged_defaults(self):
        """The model's constants the privileged row is normalised by, in the env's dtype (privileged.model_defaults)."""
        mu, pg, kv = self._envp_default
        return privileged.model_defaults(pg, self.cfg.control.decimation, mu, kv, np.float64 if self._real == torch.float64 else np.float32)

    def render(self):
        pass

    # ------------------------------------------------------------------ state access (parity tests, checkpoints)
    def get_state(self):
        N = self.num_envs
        qpos, qvel, qw = np.empty((N, 25)), np.empty((N, 24)), np.empty((N, 24))
        self._ck(self._L.nm_get_state(self._h, qpos.ctypes.data, qvel.ctypes.data, qw.ctypes.data))
        return qpos, qvel, qw

    def set_state(self, qpos=None, qvel=None, qacc_warmstart=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (qpos, qvel, qacc_warmstart)]
        self._ck(self._L.nm_set_state(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def get_buffers(self):
        N = self.num_envs
        out = dict(dof_pos=np.empty((N, 18)), dof_vel=np.empty((N, 18)), actions=np.empty((N, 18)), commands=np.empty((N, 3)),
                   episode_sums=np.empty((N, _lib.NUM_REWARDS)))
        self._ck(self._L.nm_get_buffers(self._h, *[out[k].ctypes.data for k in ("dof_pos", "dof_vel", "actions", "commands", "episode_sums")]))
        return out

    def set_buffers(self, dof_pos=None, dof_vel=None, actions=None, commands=None, episode_sums=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (dof_pos, dof_vel, actions, commands, episode_sums)]
        self._ck(self._L.nm_set_buffers(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def get_feet_state(self):
        """(feet_air_time [N,6] f64, last_contacts [N,6] u8, last_contacts_filt [N,6] u8): state of _reward_feet_air_time (:90-93)."""
        N = self.num_envs
        air, last, filt = np.empty((N, 6)), np.empty((N, 6), np.uint8), np.empty((N, 6), np.uint8)
        self._ck(self._L.nm_get_feet_state(self._h, air.ctypes.data, last.ctypes.data, filt.ctypes.data))
        return air, last, filt

    def set_feet_state(self, air=None, last=None, filt=None):
        f = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
        arrs = [f(air, np.float64), f(last, np.uint8), f(filt, np.uint8)]
        self._ck(self._L.nm_set_feet_state(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def set_command_uniforms(self, u):
        a = None if u is None else np.ascontiguousarray(u, np.float64).reshape(self.num_envs, 4)
        self._ck(self._L.nm_set_command_uniforms(self._h, None if a is None else a.ctypes.data))

    def counters(self):
        out = np.zeros(3, np.int64)
        self._ck(self._L.nm_get_counters(self._h, out.ctypes.data))
        return dict(contacts_dropped=int(out[0]), bad_state_resets=int(out[1]), hull_search_fallbacks=int(out[2]))

    def set_debug_buffer(self, t):
        self._dbg = t
        self._ck(self._L.nm_set_debug_buffer(self._h, None if t is None else t.data_ptr()))

    def accumulate_rewards_into(self, t):
        """t: float32 [num_envs] device tensor (or None = off). Every step() then adds its rewards to t inside the step kernel - the
        running return a runner keeps (`cur_reward_sum += rewards`) without a launch of its own. The caller zeroes / reads t."""
        if t is not None and (t.dtype != torch.float32 or t.numel() != self.num_envs or not t.is_contiguous() or t.device != self.obs_buf.device):
            raise ValueError("accumulate_rewards_into: contiguous float32 [num_envs] tensor on the env's device")
        self._ret_acc = t
        self._ck(self._L.nm_set_return_accumulator(self._h, None if t is None else t.data_ptr()))

    def set_step_variant(self, generic):
        """generic=True: step() always launches the generic step kernel; False (the default of a new env): the lean instantiation for the
        shipped default configuration whenever a launch qualifies (include/nightmare_hip.h nm_set_step_variant). Same bits either way."""
        self._ck(self._L.nm_set_step_variant(self._h, 1 if generic else 0))

    def step_variant(self):
        """'lean' or 'generic': what the last step() / step_physics() launched."""
        return "lean" if self._L.nm_get_step_variant(self._h) == 1 else "generic"

    def profile(self, enable):
        """(sum_ms, count) of step-kernel HIP-event times since the last call; sets event recording on/off."""
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._ck(self._L.nm_profile(self._h, int(bool(enable)), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    @property
    def commands(self):
        return self.get_buffers()["commands"]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            torch.cuda.synchronize(self.device)
            self._L.nm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
