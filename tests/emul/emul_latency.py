"""ctypes binding of the host SIMT emulation with per-env actuation latency (tests only; see nm_emul_latency.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_latency.so")
SRC = [os.path.join(HERE, "nm_emul_latency.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                                     for f in ("nm_core.h", "simt.h", "nm_host_model.h", os.path.join("..", "model", "nm_model_data.h"))]
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces"]     # tests/emul/emul.py's, so all shims round alike
H = 3


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", LIB, SRC[0]])
    return LIB


def build_program(out, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. No -g, and
    -O0 for instrumented builds: the optimiser's passes over the instrumented lockstep loops take the compiler minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_LATENCY_MAIN"] + list(extra) + ["-o", out, SRC[0]])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emull_create.restype = C.c_void_p
        L.emull_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int]
        L.emull_destroy.argtypes = [C.c_void_p]
        L.emull_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p]
        L.emull_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emull_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emull_set_latency.argtypes = [C.c_void_p, C.c_void_p]
        L.emull_hist.argtypes = [C.c_void_p]
        L.emull_hist.restype = C.POINTER(C.c_float)
        L.emull_eplen.argtypes = [C.c_void_p]
        L.emull_eplen.restype = C.POINTER(C.c_int64)
        L.emull_together_count.restype = C.c_long
        assert L.emull_lat_h() == H
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16))
DBG_NTOG, DBG_NCON = 156, 160      # words of an env's debug row (nm_core.h env_debug)


class EmulLatency:
    def __init__(self, N, double=False, seed=0, env_off=0, envs_per_wave=2):
        self.L = lib()
        self.N = N
        self.h = self.L.emull_create(N, int(double), seed, env_off, envs_per_wave)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emull_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emull_get(self.h, w, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        v = np.ascontiguousarray(val, np.float64).reshape(self.N, k)
        self.L.emull_set(self.h, w, _p(v))

    def set_action_latency(self, substeps=None):
        """[N] delays in physics substeps, or None: the launch arguments carry no rows at all (the default instantiation)."""
        d = None if substeps is None else np.ascontiguousarray(substeps, np.int32).reshape(self.N)
        self.L.emull_set_latency(self.h, _p(d))

    @property
    def history(self):
        """[N,H,18] float32 view of the env's action history, row 0 the latest."""
        return np.ctypeslib.as_array(self.L.emull_hist(self.h), (self.N, H, 18))

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emull_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emull_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False, want_dbg=False):
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        dbg = np.zeros((N, 256)) if want_dbg else None
        self.L.emull_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only), _p(dbg))
        self.dbg = dbg
        return obs, rew, done, to
