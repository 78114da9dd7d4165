"""ctypes binding of the host SIMT emulation with the lean configuration traits (tests only; see nm_emul_lean.cpp): one library that
steps the generic emulation of emul.py and the lean one, so that a test can hold them against each other."""
import ctypes as C
import os
import subprocess

from . import emul as em

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libnm_emul_lean.so")
SRC = [os.path.join(HERE, "nm_emul_lean.cpp")] + em.SRC


def build(force=False):
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-missing-braces", "-DNM_DEBUG_SOLVER",
                               "-o", LIB, SRC[0]])           # tests/emul/emul.py's flags, so both emulations round alike
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int]
        L.emul_create.restype = C.c_void_p
        L.emul_create.argtypes = [C.c_int, C.c_uint64, C.c_int64]
        L.emul_refused.argtypes = [C.c_void_p]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_step.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 3
        L.emu_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emu_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emu_set_noise.argtypes = [C.c_void_p] * 3
        L.emu_record.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emu_configure.argtypes = [C.c_void_p] * 3
        L.emu_feet.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.emu_hull_cache.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.emu_eplen.argtypes = [C.c_void_p]
        L.emu_eplen.restype = C.POINTER(C.c_int64)
        L.emu_together_count.restype = C.c_long
        _lib = L
    return _lib


class Env(em.EmulEnv):
    """fp32, two envs per wave. lean=True: wave_step on nm::CfgLean; False: the generic emulation, from the same library."""

    def __init__(self, N, lean, seed=0, env_off=0):
        self.L = lib()
        self.N = N
        self.h = self.L.emul_create(N, seed, env_off) if lean else self.L.emu_create(N, 0, seed, env_off, 2)
        self.lean = lean

    def refused(self):
        """lean only: steps that did not run because the configuration or an optional input is not the lean kernel's."""
        return self.L.emul_refused(self.h) if self.lean else 0
