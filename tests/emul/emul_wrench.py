"""ctypes binding of the host SIMT emulation with the external wrench on the base (tests only; see nm_emul_wrench.cpp): levels 0 and 7 of
the step, the wrench rows behind the torque rows, and the body rows. Layout, defaults and admission are the host object's own
(nightmare_rl_amd/csrc/nm_env_rows.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_wrench.so")
SRC = [os.path.join(HERE, "nm_emul_wrench.cpp")] + [os.path.join(HERE, "..", "..", "nightmare_rl_amd", "csrc", f)
                                                    for f in ("nm_core.h", "simt.h", "nm_host_model.h", "nm_env_rows.h", os.path.join("..", "model", "nm_model_data.h"))]
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-missing-braces"]     # tests/emul/emul.py's, so all shims round alike


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", LIB, SRC[0]])
    return LIB


def build_program(out, extra=(), opt="-O1"):
    """The shim as a stand-alone program (its own main; e.g. extra=["-fsanitize=address,undefined"]): never loaded into Python. It takes
    the states file. No -g, and -O0 for instrumented builds: the optimiser's passes over the instrumented lockstep loops take minutes."""
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-O1"] + [opt, "-DNM_EMUL_WRENCH_MAIN"] + list(extra) + ["-o", out, SRC[0]])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emux_create.restype = C.c_void_p
        L.emux_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int]
        L.emux_destroy.argtypes = [C.c_void_p]
        L.emux_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int]
        L.emux_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emux_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in (L.emux_set_wrench, L.emux_get_wrench, L.emux_set_body):
            f.argtypes = [C.c_void_p, C.c_void_p]
        L.emux_level.argtypes = [C.c_void_p, C.c_int]
        L.emux_device_layout_agrees.argtypes = [C.c_void_p]
        L.emux_eplen.argtypes = [C.c_void_p]
        L.emux_eplen.restype = C.POINTER(C.c_int64)
        L.emux_together_count.restype = C.c_long
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


WHAT = dict(qpos=(0, 25), qvel=(1, 24), qwarm=(2, 24), dofpos=(3, 18), dofvel=(4, 18), act=(5, 18), cmd=(6, 3), epsum=(7, 16))


def rows8(wrench, n):
    """[n,8] rows (F, pad, tau, pad) of [n,6] or [6] wrenches (F, tau)."""
    w = np.broadcast_to(np.asarray(wrench, np.float64), (n, 6))
    r = np.zeros((n, 8))
    r[:, 0:3], r[:, 4:7] = w[:, 0:3], w[:, 3:6]
    return r


class EmulWrench:
    def __init__(self, N, double=False, seed=0, envs_per_wave=2):
        self.L = lib()
        self.N = N
        self.h = self.L.emux_create(N, int(double), seed, envs_per_wave)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emux_destroy(self.h)
            self.h = None

    def get(self, name):
        w, k = WHAT[name]
        out = np.empty((self.N, k))
        self.L.emux_get(self.h, w, _p(out))
        return out

    def set(self, name, val):
        w, k = WHAT[name]
        v = np.ascontiguousarray(val, np.float64).reshape(self.N, k)
        self.L.emux_set(self.h, w, _p(v))

    def set_base_wrench(self, wrench=None):
        """[N,6] (F, tau) or anything that broadcasts to it, None: off. ValueError where the host's admission refuses them (nothing changes)."""
        if wrench is None:
            self.L.emux_set_wrench(self.h, None)
            return
        if self.L.emux_set_wrench(self.h, _p(np.ascontiguousarray(rows8(wrench, self.N)))):
            raise ValueError("wrench rows refused")

    def wrench_rows(self):
        """[N,8]: what the region holds, zero while the kind is off."""
        r = np.empty((self.N, 8))
        self.L.emux_get_wrench(self.h, _p(r))
        return r

    def set_body_rows(self, rows=None):
        """[N,20] body rows (nightmare_rl_amd/model/payload.py), None: the model's."""
        if rows is None:
            self.L.emux_set_body(self.h, None)
        elif self.L.emux_set_body(self.h, _p(np.ascontiguousarray(rows, np.float64).reshape(self.N, 20))):
            raise ValueError("body rows refused")

    def level(self, physics_only=False):
        return self.L.emux_level(self.h, int(physics_only))

    def device_layout_agrees(self):
        return bool(self.L.emux_device_layout_agrees(self.h))

    @property
    def eplen(self):
        return np.ctypeslib.as_array(self.L.emux_eplen(self.h), (self.N,))

    def together_count(self):
        return int(self.L.emux_together_count())

    def step(self, actions, cmd_u=None, nsub=2, physics_only=False, force_level=-1):
        N = self.N
        a = np.ascontiguousarray(actions, np.float32).reshape(N, 18)
        cu = None if cmd_u is None else np.ascontiguousarray(cmd_u, np.float64).reshape(N, 4)
        obs, rew, done, to = np.zeros((N, 66), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, np.float32)
        if self.L.emux_step(self.h, _p(a), _p(cu), _p(obs), _p(rew), _p(done), _p(to), nsub, int(physics_only), force_level):
            raise RuntimeError("the wrench shim runs levels 0 and 7 only")
        return obs, rew, done, to
