"""ctypes binding of the host SIMT emulation of the device kernel (tests only; see nm_emul.cpp): one source, one library per set of step
levels compiled in. Layout, defaults, admission and the level a launch takes are the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = [os.path.join(HERE, "nm_emul.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                             for f in ("nm_core.h", "simt.h", "nm_host_model.h", "nm_env_rows.h", os.path.join("..", "model", "nm_model_data.h"))]
# the one set of flags, so every library rounds alike; NM_DEBUG_SOLVER only adds debug words
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces", "-DNM_DEBUG_SOLVER"]
# the level sets the suite uses: a library costs about 25 s of compile time per level. BASE also holds the lean step
BASE, ROWS, SERVO, TORQUE, WRENCH = (0,), (0, 1, 2, 3, 4), (0, 5), (0, 6), (0, 7)
H = 3
FRIC, BODY, LAT, GRAV, SRV, TRQ, WRN = range(7)      # nmrows::Kind, the kinds of levels 1..7
# row widths and columns as nm_core.h has them: stated here so that shapes exist before a library is loaded, and tied to the header by
# the assert on emu_sizes in _load, which every library passes before its first use
WIDTH = {FRIC: 3, BODY: 20, GRAV: 8, SRV: 4, TRQ: 4, WRN: 8}
EP_KV, SV_RATE, SV_DGAIN, WP_F, WP_T = 2, 0, 1, 0, 4      # columns of a friction / gain, a servo and a wrench row


def mask(levels):
    return sum(1 << l for l in set(levels))


def build(levels=BASE, force=False):
    """libnm_emul_<mask>.so, built under a name of this process's own and renamed: two processes may build the same library at once."""
    out = os.path.join(HERE, "libnm_emul_%02x.so" % mask(levels))
    if force or not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in SRC):
        tmp = "%s.%d.so" % (out[:-3], os.getpid())
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-DNM_EMUL_LEVELS=%du" % mask(levels), "-o", tmp, SRC[0]])
        os.replace(tmp, out)
    return out


def build_program(out, levels, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. It takes
    the mode (envp, payload, latency, servo, torque, wrench) and the states file; `levels`: the level the mode runs. No -g, and -O0 for
    instrumented builds: the optimiser's passes over the instrumented lockstep loops take the compiler minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_MAIN", "-DNM_EMUL_LEVELS=%du" % mask(levels)] + list(extra) + ["-o", out, SRC[0]])
    return out


@functools.lru_cache(None)
def _load(m):
    L = C.CDLL(build([l for l in range(8) if m >> l & 1]))
    vp = C.c_void_p
    L.emu_create.restype = vp
    L.emu_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_int]
    L.emu_step.argtypes = [vp] * 7 + [C.c_int] * 2 + [vp] * 3 + [C.c_int]
    L.emu_array.argtypes = [vp, C.c_int, C.c_int, vp]
    L.emu_servo_state.argtypes = [vp, C.c_int, vp]
    for f in (L.emu_set_rows, L.emu_get_rows, L.emu_default_row, L.emu_record):
        f.argtypes = [vp, C.c_int, vp]
    for f in (L.emu_destroy, L.emu_layout_agrees, L.emu_refused):
        f.argtypes = [vp]
    L.emu_set_noise.argtypes = L.emu_configure.argtypes = [vp] * 3
    L.emu_feet.argtypes = [vp, C.c_int, vp, vp]
    L.emu_hull_cache.argtypes = [vp, C.c_int, vp]
    L.emu_flags.argtypes = [vp] * 4
    L.emu_hist.argtypes = L.emu_eplen.argtypes = [vp]
    L.emu_hist.restype = C.POINTER(C.c_float)
    L.emu_eplen.restype = C.POINTER(C.c_int64)
    L.emu_together_count.restype = C.c_long
    L.emu_levels.restype = C.c_uint
    sizes = np.zeros(14, np.int32)
    L.emu_sizes(_p(sizes))
    assert L.emu_levels() == m
    assert sizes.tolist() == [len(REW_NAMES), 256, H] + [WIDTH[k] for k in (FRIC, BODY, GRAV, SRV, TRQ, WRN)] + [EP_KV, SV_RATE, SV_DGAIN, WP_F, WP_T]
    return L


def lib(levels=BASE):
    return _load(mask(levels))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16),
            feetair=(8, 6), feetflags=(9, 1), hcache=(10, 8), rngctr=(11, 1))      # the last four: what else a step carries over
DBG_NTOG, DBG_NCON, DBG_NWARN = 156, 160, 161      # words of an env's debug row (nm_core.h env_debug)
REW_NAMES = ["action_rate", "ang_vel_xy", "base_height", "body_contact_forces", "default_position", "dof_acc", "dof_vel", "feet_air_time",
             "feet_contact_forces", "lin_vel_z", "orientation", "stand_still", "torques", "tracking_ang_vel", "tracking_lin_vel", "termination"]


def rows8(wrench, n):
    """[n,8] rows (F, pad, tau, pad) of [n,6] or [6] wrenches (F, tau)."""
    w = np.broadcast_to(np.asarray(wrench, np.float64), (n, 6))
    r = np.zeros((n, WIDTH[WRN]))
    r[:, WP_F:WP_F + 3], r[:, WP_T:WP_T + 3] = w[:, 0:3], w[:, 3:6]
    return r


class EmulEnv:
    """One env object of the shim, from the library of the class's `levels`. lean=True (fp32, two envs per wave, level 0 in the library):
    wave_step on nm::CfgLean, which refuses (refused()) what the host refuses for the lean kernel."""
    levels = BASE

    def __init__(self, N, double=False, seed=0, env_off=0, envs_per_wave=2, lean=False):
        self.L = lib(self.levels)
        self.N = N
        self.lean = lean
        self.h = self.L.emu_create(N, int(double), seed, env_off, envs_per_wave, int(lean))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emu_array(self.h, w, 0, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        self.L.emu_array(self.h, w, 1, _p(np.ascontiguousarray(val, np.float64).reshape(self.N, k)))

    # ---- the per-env rows. Every setter: rows, or None = off; ValueError where the host's admission refuses them (nothing changes)
    def _set_rows(self, kind, rows, what):
        r = None if rows is None else np.ascontiguousarray(rows, np.int32 if kind == LAT else np.float64).reshape((self.N,) if kind == LAT else (self.N, WIDTH[kind]))
        if self.L.emu_set_rows(self.h, kind, _p(r)):
            raise ValueError(what + " rows refused")

    def _rows(self, kind):
        """What the region holds, whatever is on: the defaults of a kind that is off."""
        out = np.zeros(self.N, np.int32) if kind == LAT else np.zeros((self.N, WIDTH[kind]))
        assert self.L.emu_get_rows(self.h, kind, _p(out)) == 0
        return out

    def set_env_params(self, rows=None):
        """[N,3] rows (mu, p_gain, kv)."""
        self._set_rows(FRIC, rows, "friction")

    def set_body_params(self, rows=None):
        """[N,20] body rows (nightmare_rl_amd.model.payload.payload_rows)."""
        self._set_rows(BODY, rows, "body")

    def set_action_latency(self, substeps=None):
        """[N] delays in physics substeps."""
        self._set_rows(LAT, substeps, "latency")

    def set_gravity(self, rows=None):
        """[N,8] rows (g[3], pad, gravity_vec[3], pad)."""
        self._set_rows(GRAV, rows, "gravity")

    set_body_rows = set_body_params

    def set_kv(self, kv=None):
        """[N] kv (a scalar: every env) in the default friction / gain rows, which turns that kind on; None: the default rows, off."""
        self.set_env_params()
        if kv is not None:
            r = self._rows(FRIC)
            r[:, EP_KV] = kv
            self.set_env_params(r)

    def set_servo(self, rate=None, d_gain=None):
        """[N] rates and d_gains (scalars: every env; one of them None: its default, inf or 0), or both None: off."""
        r = None if rate is None and d_gain is None else np.zeros((self.N, WIDTH[SRV]))
        if r is not None:
            r[:, SV_RATE], r[:, SV_DGAIN] = np.inf if rate is None else rate, 0.0 if d_gain is None else d_gain
        self._set_rows(SRV, r, "servo")

    def servo(self):
        """([N] rate, [N] d_gain): what the region holds, the defaults (inf, 0) while the kind is off."""
        r = self._rows(SRV)
        return r[:, SV_RATE].copy(), r[:, SV_DGAIN].copy()

    def servo_state(self):
        """[N,18] the servo's limited targets: state, like the history."""
        out = np.empty((self.N, 18))
        self.L.emu_servo_state(self.h, 0, _p(out))
        return out

    def set_servo_state(self, lim):
        self.L.emu_servo_state(self.h, 1, _p(np.ascontiguousarray(lim, np.float64).reshape(self.N, 18)))

    def set_torque_limit(self, limit=None):
        """[N,3] limits (or anything that broadcasts to it), None: off."""
        r = None if limit is None else np.zeros((self.N, WIDTH[TRQ]))
        if r is not None:
            r[:, :3] = limit
        self._set_rows(TRQ, r, "torque")

    def torque_rows(self):
        """[N,4]: what the region holds, (inf, inf, inf, 0) while the kind is off."""
        return self._rows(TRQ)

    def set_base_wrench(self, wrench=None):
        """[N,6] (F, tau) or anything that broadcasts to it, None: off."""
        self._set_rows(WRN, None if wrench is None else rows8(wrench, self.N), "wrench")

    def wrench_rows(self):
        """[N,8]: what the region holds, zero while the kind is off."""
        return self._rows(WRN)

    def default_body_row(self):
        """The model's own body row in the env's precision: what nm_get_body_params reports while the feature is off."""
        out = np.zeros(20)
        assert self.L.emu_default_row(self.h, BODY, _p(out)) == 0
        return out

    default_row = default_body_row

    def rows(self):
        """([N,3] friction / gains, [N,20] body rows, [N] delays, [N,8] gravity rows)."""
        return tuple(self._rows(k) for k in (FRIC, BODY, LAT, GRAV))

    def gravity(self):
        return self._rows(GRAV)

    def _flags(self):
        on, lv, c = np.zeros(7, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)
        self.L.emu_flags(self.h, _p(on), _p(lv), _p(c))
        return on, lv, bool(c[0])

    def state(self, physics_only=False):
        """(kinds that are on as a string of F, B, L, G; the level a launch takes)."""
        return "".join(k for i, k in enumerate("FBLG") if self._flags()[0][i]), self.level(physics_only)

    def level(self, physics_only=False):
        return int(self._flags()[1][int(physics_only)])

    def carries_block(self):
        """Whether a launch carries the block at all (nm::Args::envp non-null)."""
        return self._flags()[2]

    def layout_agrees(self):
        """The device's accessors, the host's and the layout agree over the whole block, and the regions tile it (nm_emul.cpp)."""
        return bool(self.L.emu_layout_agrees(self.h))

    @property
    def history(self):
        """[N,H,18] float32 view of the env's action history, row 0 the latest."""
        return np.ctypeslib.as_array(self.L.emu_hist(self.h), (self.N, H, 18))

    # ---- configuration, feet, hull cache, noise, the state log
    def configure(self, reward_scales, tibia_contact_mode=1, tibia_max_contact_force=2.0, body_contact_mode=1, body_max_contact_force=2.0,
                  base_height_target=0.1, max_contact_force=10.0):
        sc = np.array([float(reward_scales.get(n, 0.0)) for n in REW_NAMES])
        m = np.array([tibia_contact_mode, tibia_max_contact_force, body_contact_mode, body_max_contact_force, base_height_target, max_contact_force], np.float64)
        self.L.emu_configure(self.h, _p(sc), _p(m))

    def get_feet_state(self):
        air, fl = np.zeros((self.N, 6)), np.zeros(self.N, np.int32)
        self.L.emu_feet(self.h, 0, _p(air), _p(fl))
        bits = (fl[:, None] >> np.arange(12)[None, :]) & 1
        return air, bits[:, :6].astype(np.uint8), bits[:, 6:].astype(np.uint8)

    def set_feet_state(self, air, last, filt):
        air = np.ascontiguousarray(air, np.float64)
        fl = ((np.asarray(last, np.int32) << np.arange(6)).sum(1) | (np.asarray(filt, np.int32) << (6 + np.arange(6))).sum(1)).astype(np.int32)
        self.L.emu_feet(self.h, 1, _p(air), _p(fl))

    def hull_cache(self, value=None):
        """[N,8] ints: warm-start vertex of the 7 colliding meshes + the env's running exhaustive-scan count; set when `value` given."""
        hc = np.zeros((self.N, 8), np.int32) if value is None else np.ascontiguousarray(value, np.int32).reshape(self.N, 8)
        self.L.emu_hull_cache(self.h, int(value is not None), _p(hc))
        return hc

    def set_noise(self, vec=None, u=None):
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
        vec, u = f(vec), f(u)
        self.L.emu_set_noise(self.h, _p(vec), _p(u))

    def record(self, env):
        """Select the env whose pre-reset state is logged; returns the last record (qpos25, qvel24, nbad)."""
        out = np.zeros(50)
        self.L.emu_record(self.h, env, _p(out))
        return out[:25], out[25:49], int(out[49])

    def refused(self):
        """lean only: steps that did not run because the configuration or an optional input is not the lean kernel's."""
        return self.L.emu_refused(self.h)

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emu_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emu_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False, want_dbg=False, force_level=-1):
        """At the level the host chooses from what is on, or default rows through force_level's code. RuntimeError for a level that the
        library does not hold."""
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        dbg = np.zeros((N, 256)) if want_dbg else None
        ssum, scnt = np.zeros(16), np.zeros(2, np.int32)
        if self.L.emu_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only), _p(dbg), _p(ssum), _p(scnt), force_level):
            raise RuntimeError("the library holds levels of mask %#x only" % self.L.emu_levels())
        self.dbg, self.stat_sum, self.stat_cnt = dbg, ssum, scnt
        return obs, rew, done, to


class EmulRows(EmulEnv):
    """The same env from the library that holds levels 0..4."""
    levels = ROWS


class EmulServo(EmulEnv):
    levels = SERVO


class EmulTorque(EmulEnv):
    levels = TORQUE


class EmulWrench(EmulEnv):
    levels = WRENCH
