"""ctypes binding of the host SIMT emulation with the per-env rows of nm::Args::envp: friction / gains, body rows (base payload), actuation
latency, gravity vectors (tests only; see nm_emul_rows.cpp). One shim for the four kinds: layout, defaults, admission, state and level are
the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_rows.so")
SRC = [os.path.join(HERE, "nm_emul_rows.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                                  for f in ("nm_core.h", "simt.h", "nm_host_model.h", "nm_env_rows.h", os.path.join("..", "model", "nm_model_data.h"))]
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces"]     # tests/emul/emul.py's, so both shims round alike
H = 3


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", LIB, SRC[0]])
    return LIB


def build_program(out, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. It takes
    the mode (envp, payload, latency) and the states file. No -g, and -O0 for instrumented builds: the optimiser's passes over the
    instrumented lockstep loops take the compiler minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_ROWS_MAIN"] + list(extra) + ["-o", out, SRC[0]])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emur_create.restype = C.c_void_p
        L.emur_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int]
        L.emur_destroy.argtypes = [C.c_void_p]
        L.emur_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p]
        L.emur_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emur_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in (L.emur_set_envp, L.emur_set_body, L.emur_set_latency, L.emur_set_gravity, L.emur_default_body_row, L.emur_on_flags):
            f.argtypes = [C.c_void_p, C.c_void_p]
        L.emur_get_rows.argtypes = [C.c_void_p] * 5
        L.emur_level.argtypes = [C.c_void_p, C.c_int]
        L.emur_carries_block.argtypes = [C.c_void_p]
        L.emur_device_layout_agrees.argtypes = [C.c_void_p]
        L.emur_hist.argtypes = [C.c_void_p]
        L.emur_hist.restype = C.POINTER(C.c_float)
        L.emur_eplen.argtypes = [C.c_void_p]
        L.emur_eplen.restype = C.POINTER(C.c_int64)
        L.emur_together_count.restype = C.c_long
        assert L.emur_lat_h() == H and L.emur_grav_p() == 8
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16),
            feetair=(8, 6), feetflags=(9, 1), hcache=(10, 8), rngctr=(11, 1))      # the last four: what else a step carries over
DBG_NTOG, DBG_NCON, DBG_NWARN = 156, 160, 161      # words of an env's debug row (nm_core.h env_debug)


class EmulRows:
    def __init__(self, N, double=False, seed=0, env_off=0, envs_per_wave=2):
        self.L = lib()
        self.N = N
        self.h = self.L.emur_create(N, int(double), seed, env_off, envs_per_wave)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emur_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emur_get(self.h, w, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        v = np.ascontiguousarray(val, np.float64).reshape(self.N, k)
        self.L.emur_set(self.h, w, _p(v))

    def set_env_params(self, rows=None):
        """[N,3] rows (mu, p_gain, kv), or None: off (the launch arguments carry no rows at all unless another kind is on)."""
        r = None if rows is None else np.ascontiguousarray(rows, np.float64).reshape(self.N, 3)
        self.L.emur_set_envp(self.h, _p(r))

    def set_body_params(self, rows=None):
        """[N,20] body rows (nightmare_rl_amd.model.payload.payload_rows), or None: off. ValueError where the host's admission refuses
        them (nothing changes)."""
        r = None if rows is None else np.ascontiguousarray(rows, np.float64).reshape(self.N, 20)
        if self.L.emur_set_body(self.h, _p(r)):
            raise ValueError("body rows refused")

    def set_action_latency(self, substeps=None):
        """[N] delays in physics substeps, or None: off."""
        d = None if substeps is None else np.ascontiguousarray(substeps, np.int32).reshape(self.N)
        self.L.emur_set_latency(self.h, _p(d))

    def set_gravity(self, rows=None):
        """[N,8] rows (g[3], pad, gravity_vec[3], pad) or None: off. ValueError where the host's admission refuses them (nothing changes)."""
        r = None if rows is None else np.ascontiguousarray(rows, np.float64).reshape(self.N, 8)
        if self.L.emur_set_gravity(self.h, _p(r)):
            raise ValueError("gravity rows refused")

    def default_body_row(self):
        """The model's own body row in the env's precision: what nm_get_body_params reports while the feature is off."""
        out = np.zeros(20)
        self.L.emur_default_body_row(self.h, _p(out))
        return out

    default_row = default_body_row

    def rows(self):
        """What the block holds, whatever is on (the defaults of a kind that is off): ([N,3] friction / gains, [N,20] body rows, [N] delays,
        [N,8] gravity rows)."""
        e, b, d, g = np.zeros((self.N, 3)), np.zeros((self.N, 20)), np.zeros(self.N, np.int32), np.zeros((self.N, 8))
        self.L.emur_get_rows(self.h, _p(e), _p(b), _p(d), _p(g))
        return e, b, d, g

    def gravity(self):
        """What the gravity region holds, whatever is on: the defaults while the kind is off."""
        return self.rows()[3]

    def state(self, physics_only=False):
        """(kinds that are on as a string of F, B, L, G; the level a launch takes)."""
        on = np.zeros(4, np.int32)
        self.L.emur_on_flags(self.h, _p(on))
        return "".join(k for i, k in enumerate("FBLG") if on[i]), self.L.emur_level(self.h, int(physics_only))

    def carries_block(self):
        """Whether a launch carries the block at all (nm::Args::envp non-null)."""
        return bool(self.L.emur_carries_block(self.h))

    def device_layout_agrees(self):
        return bool(self.L.emur_device_layout_agrees(self.h))

    @property
    def history(self):
        """[N,H,18] float32 view of the env's action history, row 0 the latest."""
        return np.ctypeslib.as_array(self.L.emur_hist(self.h), (self.N, H, 18))

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emur_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emur_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False, want_dbg=False):
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        dbg = np.zeros((N, 256)) if want_dbg else None
        self.L.emur_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only), _p(dbg))
        self.dbg = dbg
        return obs, rew, done, to
