"""The cross-lane helpers that the lean step kernel takes in another form than the generic kernels (csrc/simt.h): the half-wave row
broadcast of the two-env constraint pass as two DPP moves (fma_half_lane_dpp) against two v_readlane, two moves and a select
(fma_half_lane), and the walking lane-mask select as a compiler-visible instruction (sel_mask_open) against the inline-asm one
(sel_mask). Both forms of each helper run side by side on the same values (csrc/nm_lane_selftest.h: nm_lane_selftest on the device, the
same lines on the host emulation of simt.h) and must agree lane for lane and bit for bit - they only move data; where the arithmetic
is exact (a = 1, g = -0) the result must also be the gather it stands for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SLOTS, NMASK = 36, 4
SIZES = [64, 130]          # one wave; three waves, the last with two lanes
# lane masks of the sweeps: a row of one env, the same row of both halves, a pair of both halves, and one with most lanes masked off
MASKS = [[1 << 5, 0x0000000100000001 << 7, 0x0000000300000003 << 12, 0x8000000000000001],
         [0, (1 << 64) - 1, 0x00000000ffffffff, 0xaaaaaaaa55555555]]


def _values(n, seed):
    """name -> x [n] float32: the values a row broadcast meets, and the ones it must not mangle."""
    r = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)
    tiny = f(np.frombuffer(r.integers(1, 1 << 23, n, dtype=np.uint32).tobytes(), np.float32))        # denormals, every mantissa
    ties = f(r.normal(size=n)); ties[::7] = ties[3]; ties[5::11] = ties[3]                              # the same value in several lanes
    zeros = f(np.where(r.random(n) < 0.5, 0.0, -0.0))
    infs = f(r.normal(size=n)); infs[::5] = np.inf; infs[2::9] = -np.inf
    nans = f(r.normal(size=n)); nans[1::6] = np.nan; nans[4::13] = -np.nan                                # quiet NaNs in some lanes
    sent = f(r.normal(size=n)); sent[r.random(n) < 0.6] = -1e30                                       # the hull search's "no candidate"
    return {"random": f(r.normal(size=n) * 10 ** r.uniform(-6, 6, n)), "equal": np.full(n, 0.37, np.float32), "ties": ties, "zeros": zeros,
            "denormal": np.where(r.random(n) < 0.5, tiny, -tiny).astype(np.float32), "inf": infs, "nan": nans, "sentinel": sent}


def _cases():
    for n in SIZES:
        for k, (name, x) in enumerate(_values(n, 100 + n).items()):
            r = np.random.default_rng(7 * n + k)
            yield f"{name}-{n}-move", x, np.ones(n, np.float32), np.full(n, -0.0, np.float32), MASKS[k % 2], True
            yield f"{name}-{n}-fma", x, r.normal(size=n).astype(np.float32), r.normal(size=n).astype(np.float32), MASKS[(k + 1) % 2], False


def _gather(x, n):
    """[32, n]: x of lane I of the lane's own half-wave, zeros behind n (what the waves' idle lanes hold)."""
    xp = np.zeros((n + 63) // 64 * 64, np.float32)
    xp[:n] = x
    i = np.arange(n)
    return np.stack([xp[(i & ~31) + I] for I in range(32)])


def _check(out, x, a, g, masks, exact, n, tag):
    out = out.reshape(2, SLOTS, n)
    bits = out.view(np.uint32)
    np.testing.assert_array_equal(bits[0], bits[1], err_msg=f"{tag}: the lean form differs from the form it replaces")
    lane = np.arange(n) % 64
    for k, m in enumerate(masks):
        want = np.where(np.array([(m >> int(l)) & 1 for l in lane], bool), a, g).astype(np.float32)
        np.testing.assert_array_equal(bits[0, 32 + k], want.view(np.uint32), err_msg=f"{tag}: mask {m:#x}")
    if exact:       # 1 * x + (-0) is x itself, sign of zero and denormals included; a NaN stays a NaN
        want = _gather(x, n)
        assert np.array_equal(np.isnan(out[0, :32]), np.isnan(want)), tag
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(bits[0, :32][ok], want.view(np.uint32)[ok], err_msg=f"{tag}: not the half-wave gather")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lane") / "liblane_selftest_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "lane_selftest_emul.cpp")])
    L = C.CDLL(out)
    L.lane_selftest_emul.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    return L


def test_host_emulation_forms_agree(emul):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for tag, x, a, g, masks, exact in _cases():
        n = len(x)
        out = np.full(2 * SLOTS * n, 7.0, np.float32)
        m = np.array(masks, np.uint64)
        assert emul.lane_selftest_emul(p(x), p(a), p(g), p(m), n, p(out)) == 0
        _check(out, x, a, g, masks, exact, n, "host " + tag)


@pytest.mark.gpu
def test_device_forms_agree():
    import torch

    from nightmare_rl_amd import _lib
    L = _lib.load()
    for tag, x, a, g, masks, exact in _cases():
        n = len(x)
        xd, ad, gd = (torch.from_numpy(v).cuda() for v in (x, a, g))
        out = torch.full((2 * SLOTS * n,), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m = (C.c_uint64 * NMASK)(*masks)
        assert L.nm_lane_selftest(xd.data_ptr(), ad.data_ptr(), gd.data_ptr(), C.byref(m), n, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        _check(out.cpu().numpy(), x, a, g, masks, exact, n, "device " + tag)
