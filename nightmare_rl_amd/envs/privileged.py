"""The privileged critic row of an asymmetric actor-critic: its column names and a numpy restatement of what the device gathers
(csrc/nm_priv_obs.h k_priv_obs; include/nightmare_hip.h nm_privileged_obs). Pure Python, importable without a GPU.

Row [66 + 23]: the observation the step returned, then NAMES in order. Switched on by `cfg.env.privileged_obs = True` (a user subclass
adds the attribute, as with `domain_rand`); the env then hands the row out from step()'s second slot, get_privileged_observations() and
reset(), and the critic may read it while the actor keeps the 66-wide observation."""
import numpy as np

NUM_OBS = 66
NAMES = ("friction", "p_gain_ratio", "kv_ratio", "payload_mass", "payload_com_x", "payload_com_y", "payload_com_z", "latency_steps",
         "gravity_x", "gravity_y", "gravity_z", "servo_inv_rate", "servo_d_gain",
         "inv_torque_limit_coxa", "inv_torque_limit_femur", "inv_torque_limit_tibia",
         "wrench_force_x", "wrench_force_y", "wrench_force_z", "wrench_torque_x", "wrench_torque_y", "wrench_torque_z", "base_height")
NUM_PRIVILEGED = len(NAMES)
NUM_PRIVILEGED_OBS = NUM_OBS + NUM_PRIVILEGED
GRAVITY = 9.81


def enabled(cfg):
    """Is the switch on in this config tree? (`NightmareV3Config` has no such attribute: off.)"""
    return bool(getattr(getattr(cfg, "env", None), "privileged_obs", False))


def model_defaults(p_gain, decimation, mu, kv, real=np.float32):
    """The model's own constants the row is normalised by, rounded to the env's dtype `real` as the library holds them: p_gain (the
    config's), kv and mu (the model's: what env_params() reports while the feature is off), the base body's mass and COM offset, the
    total mass, gravity, and the decimation."""
    from ..model import compile_model as cm
    T = cm.load_tables()
    r = lambda x: np.asarray(x, np.float64).astype(real).astype(np.float64)
    return dict(mu=float(r(mu)), p_gain=float(r(p_gain)), kv=float(r(kv)), base_mass=float(r(T["body_mass"][1])), base_ipos=r(T["body_ipos"][1]),
                total_mass=float(r(np.sum(np.asarray(T["body_mass"], np.float64)[1:]))), grav=float(r(GRAVITY)), decimation=int(decimation))


def default_values(defaults):
    """The 22 parameter columns of an env none of whose rows was ever set (every kind's default row), without base_height."""
    v = np.zeros(NUM_PRIVILEGED - 1)
    v[0], v[1], v[2], v[10] = defaults["mu"], 1.0, 1.0, -1.0
    return v


def privileged_reference(obs, defaults, *, base_height, mu=None, p_gain=None, kv=None, body_rows=None, latency=None, g=None, rate_limit=None,
                         d_gain=None, torque_limit=None, force=None, torque=None):
    """float32 [N, 89]: `obs` [N, 66] followed by the 23 columns of NAMES, from what the env's getters report - mu / p_gain / kv [N]
    (env_params()), body_rows [N, 20] (base_payload()['rows']), latency [N] substeps (action_latency()), g [N, 3] (gravity()['g']),
    rate_limit / d_gain [N] (servo()), torque_limit [N, 3] (torque_limit()), force / torque [N, 3] (base_wrench()) - and base_height [N]
    (qpos[:, 2]). None = that kind's default row. defaults: model_defaults(). The arithmetic is float64 on the getters' values, rounded to
    float32 once - what the kernel does."""
    obs = np.asarray(obs, np.float32)
    N = obs.shape[0]
    f = lambda x, shape: None if x is None else np.broadcast_to(np.asarray(x, np.float64), shape)
    d = defaults
    out = np.empty((N, NUM_PRIVILEGED), np.float64)
    out[:, :22] = default_values(d)
    with np.errstate(divide="ignore"):
        if mu is not None:
            out[:, 0] = f(mu, (N,))
        if p_gain is not None:
            out[:, 1] = f(p_gain, (N,)) / d["p_gain"]
        if kv is not None:
            out[:, 2] = f(kv, (N,)) / d["kv"]
        if body_rows is not None:
            rows = f(body_rows, (N, 20))
            out[:, 3] = rows[:, 9] - d["base_mass"]
            out[:, 4:7] = rows[:, 0:3] - np.asarray(d["base_ipos"], np.float64)
        if latency is not None:
            out[:, 7] = f(latency, (N,)) / float(d["decimation"])
        if g is not None:
            out[:, 8:11] = f(g, (N, 3)) / d["grav"]
        if rate_limit is not None:
            out[:, 11] = 1.0 / f(rate_limit, (N,))          # 1 / inf = 0
        if d_gain is not None:
            out[:, 12] = f(d_gain, (N,))
        if torque_limit is not None:
            out[:, 13:16] = 1.0 / f(torque_limit, (N, 3))
        w = d["total_mass"] * d["grav"]
        if force is not None:
            out[:, 16:19] = f(force, (N, 3)) / w
        if torque is not None:
            out[:, 19:22] = f(torque, (N, 3)) / w
    out[:, 22] = f(base_height, (N,))
    return np.concatenate([obs, out.astype(np.float32)], axis=1)
