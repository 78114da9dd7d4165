"""ctypes binding of the host SIMT emulation with per-env body rows (base payload; tests only; see nm_emul_payload.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_payload.so")
SRC = [os.path.join(HERE, "nm_emul_payload.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                                  for f in ("nm_core.h", "simt.h", "nm_host_model.h", os.path.join("..", "model", "nm_model_data.h"))]
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces"]     # tests/emul/emul.py's, so both shims round alike


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", LIB, SRC[0]])
    return LIB


def build_program(out, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. No -g, and
    -O0 for instrumented builds: the optimiser's passes over the instrumented lockstep loops take the compiler minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_PAYLOAD_MAIN"] + list(extra) + ["-o", out, SRC[0]])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emub_create.restype = C.c_void_p
        L.emub_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int]
        L.emub_destroy.argtypes = [C.c_void_p]
        L.emub_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p]
        L.emub_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emub_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emub_set_envp.argtypes = [C.c_void_p, C.c_void_p]
        L.emub_set_body.argtypes = [C.c_void_p, C.c_void_p]
        L.emub_default_row.argtypes = [C.c_void_p, C.c_void_p]
        L.emub_eplen.argtypes = [C.c_void_p]
        L.emub_eplen.restype = C.POINTER(C.c_int64)
        L.emub_together_count.restype = C.c_long
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16))
DBG_NTOG, DBG_NCON = 156, 160      # words of an env's debug row (nm_core.h env_debug)


class EmulPayload:
    def __init__(self, N, double=False, seed=0, env_off=0, envs_per_wave=2):
        self.L = lib()
        self.N = N
        self.h = self.L.emub_create(N, int(double), seed, env_off, envs_per_wave)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emub_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emub_get(self.h, w, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        v = np.ascontiguousarray(val, np.float64).reshape(self.N, k)
        self.L.emub_set(self.h, w, _p(v))

    def set_env_params(self, rows=None):
        """[N,3] rows (mu, p_gain, kv), or None: the launch arguments carry no parameter rows at all."""
        r = None if rows is None else np.ascontiguousarray(rows, np.float64).reshape(self.N, 3)
        self.L.emub_set_envp(self.h, _p(r))

    def set_body_params(self, rows=None):
        """[N,20] body rows (nightmare_rl_amd.model.payload.payload_rows), or None: off."""
        r = None if rows is None else np.ascontiguousarray(rows, np.float64).reshape(self.N, 20)
        self.L.emub_set_body(self.h, _p(r))

    def default_row(self):
        """The model's own row in the env's precision: what nm_get_body_params reports while the feature is off."""
        out = np.zeros(20)
        self.L.emub_default_row(self.h, _p(out))
        return out

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emub_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emub_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False, want_dbg=False):
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        dbg = np.zeros((N, 256)) if want_dbg else None
        self.L.emub_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only), _p(dbg))
        self.dbg = dbg
        return obs, rew, done, to
