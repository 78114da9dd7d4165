"""ctypes binding of the host SIMT emulation with the servo target model (tests only; see nm_emul_servo.cpp): levels 0 and 5 of the step,
the servo rows and the limited targets behind the gravity rows, actuation delays and the action history in front of them. Layout, defaults
and admission are the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_servo.so")
SRC = [os.path.join(HERE, "nm_emul_servo.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                                   for f in ("nm_core.h", "simt.h", "nm_host_model.h", "nm_env_rows.h", os.path.join("..", "model", "nm_model_data.h"))]
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces"]     # tests/emul/emul.py's, so all shims round alike
H = 3


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", LIB, SRC[0]])
    return LIB


def build_program(out, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. It takes
    the states file. No -g, and -O0 for instrumented builds: the optimiser's passes over the instrumented lockstep loops take minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_SERVO_MAIN"] + list(extra) + ["-o", out, SRC[0]])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emus_create.restype = C.c_void_p
        L.emus_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int]
        L.emus_destroy.argtypes = [C.c_void_p]
        L.emus_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int]
        L.emus_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emus_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in (L.emus_set_servo, L.emus_get_servo, L.emus_set_latency, L.emus_get_lim, L.emus_set_lim):
            f.argtypes = [C.c_void_p, C.c_void_p]
        L.emus_level.argtypes = [C.c_void_p, C.c_int]
        L.emus_device_layout_agrees.argtypes = [C.c_void_p]
        L.emus_hist.argtypes = [C.c_void_p]
        L.emus_hist.restype = C.POINTER(C.c_float)
        L.emus_eplen.argtypes = [C.c_void_p]
        L.emus_eplen.restype = C.POINTER(C.c_int64)
        L.emus_together_count.restype = C.c_long
        assert L.emus_lat_h() == H
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16))


class EmulServo:
    def __init__(self, N, double=False, seed=0, envs_per_wave=2):
        self.L = lib()
        self.N = N
        self.h = self.L.emus_create(N, int(double), seed, envs_per_wave)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emus_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emus_get(self.h, w, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        v = np.ascontiguousarray(val, np.float64).reshape(self.N, k)
        self.L.emus_set(self.h, w, _p(v))

    def set_servo(self, rate=None, d_gain=None):
        """[N] rates and d_gains (scalars: every env), or both None: off. ValueError where the host's admission refuses them (nothing changes)."""
        if rate is None and d_gain is None:
            self.L.emus_set_servo(self.h, None)
            return
        r = np.empty((self.N, 2))
        r[:, 0] = np.inf if rate is None else rate
        r[:, 1] = 0.0 if d_gain is None else d_gain
        if self.L.emus_set_servo(self.h, _p(r)):
            raise ValueError("servo rows refused")

    def servo(self):
        """([N] rate, [N] d_gain): what the region holds, the defaults (inf, 0) while the kind is off."""
        r = np.empty((self.N, 2))
        self.L.emus_get_servo(self.h, _p(r))
        return r[:, 0].copy(), r[:, 1].copy()

    def set_action_latency(self, substeps=None):
        d = None if substeps is None else np.ascontiguousarray(substeps, np.int32).reshape(self.N)
        self.L.emus_set_latency(self.h, _p(d))

    def servo_state(self):
        out = np.empty((self.N, 18))
        self.L.emus_get_lim(self.h, _p(out))
        return out

    def set_servo_state(self, lim):
        self.L.emus_set_lim(self.h, _p(np.ascontiguousarray(lim, np.float64).reshape(self.N, 18)))

    def level(self, physics_only=False):
        return self.L.emus_level(self.h, int(physics_only))

    def device_layout_agrees(self):
        return bool(self.L.emus_device_layout_agrees(self.h))

    @property
    def history(self):
        """[N,H,18] float32 view of the env's action history, row 0 the latest."""
        return np.ctypeslib.as_array(self.L.emus_hist(self.h), (self.N, H, 18))

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emus_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emus_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False):
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        if self.L.emus_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only)):
            raise RuntimeError("the servo shim runs levels 0 and 5 only")
        return obs, rew, done, to
