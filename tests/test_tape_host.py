"""nm_step_tape / nm_nik_tape: the C ABI against its ctypes binding, and the refusals that need no device (no GPU: nothing here launches)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def test_library_exports_the_tape_entry_points(L):
    from nightmare_rl_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_step_tape", "nm_nik_tape"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS


_C = """#include <stddef.h>
#include <stdio.h>
#include "nightmare_hip.h"
#define F(S, f) printf(#S "." #f " %%zu\\n", offsetof(S, f))
int main(void) {
  printf("nm_tape_args %%zu\\n", sizeof(nm_tape_args));
  %s
  printf("nm_nik_tape_args %%zu\\n", sizeof(nm_nik_tape_args));
  %s
  return 0;
}
"""


def test_ctypes_structs_have_the_layout_of_the_c_structs(tmp_path):
    """sizeof and every field offset of NmTapeArgs / NmNikTapeArgs = the C structs', as the host compiler lays them out."""
    from nightmare_rl_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    pairs = (("nm_tape_args", _lib.NmTapeArgs), ("nm_nik_tape_args", _lib.NmNikTapeArgs))
    lines = ["\n  ".join(f"F({cn}, {f});" for f, _ in cls._fields_) for cn, cls in pairs]
    src = tmp_path / "layout.c"
    src.write_text(_C % tuple(lines))
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got = dict((k, int(v)) for k, v in (ln.split() for ln in out.strip().splitlines()))
    for cn, cls in pairs:
        assert got[cn] == ctypes.sizeof(cls), (cn, got[cn], ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            assert got[f"{cn}.{f}"] == getattr(cls, f).offset, (cn, f, got[f"{cn}.{f}"], getattr(cls, f).offset)
    assert len(got) == 2 + sum(len(cls._fields_) for _, cls in pairs)
    # every member the header declares is bound: count the declarators of each struct in the header
    assert len(_lib.NmTapeArgs._fields_) == 19 and len(_lib.NmNikTapeArgs._fields_) == 15


def test_null_handle_and_null_args_are_refused_by_name(L):
    """Both entry points return nonzero for a NULL handle or NULL args before any device call; nm_last_error names the entry point."""
    from nightmare_rl_amd import _lib
    ta, na = _lib.NmTapeArgs(), _lib.NmNikTapeArgs()
    ta.steps = na.steps = 1
    assert L.nm_step_tape(None, ctypes.byref(ta), None) != 0
    assert b"nm_step_tape" in L.nm_last_error()
    assert L.nm_step_tape(None, None, None) != 0
    assert b"nm_step_tape" in L.nm_last_error()
    assert L.nm_nik_tape(None, ctypes.byref(na), None) != 0
    assert b"nm_nik_tape" in L.nm_last_error()
    assert L.nm_nik_tape(None, None, None) != 0
    assert b"nm_nik_tape" in L.nm_last_error()
    # a handle with NULL args: the pointer is never dereferenced before the check, so any non-NULL value serves
    dummy = ctypes.create_string_buffer(4096)
    assert L.nm_nik_tape(ctypes.cast(dummy, ctypes.c_void_p), None, None) != 0
    assert b"nm_nik_tape" in L.nm_last_error() and b"args" in L.nm_last_error()
    assert L.nm_step_tape(ctypes.cast(dummy, ctypes.c_void_p), None, None) != 0
    assert b"nm_step_tape" in L.nm_last_error() and b"args" in L.nm_last_error()
