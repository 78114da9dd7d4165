"""The sensor model's one definition - nm::sensor_apply of csrc/nm_sensor.h, the function k_sensor and the K-step launches call - compiled
for the host (simt.h under NM_EMUL, as tests/test_lane_helpers.py builds its shim) and run over a sequence of true observations, against
the numpy restatement of the three rules (tests/sensor_np.py). Copy, one float32 add and a clamp: equality is bit equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sensor_np as sn

HERE = os.path.dirname(os.path.abspath(__file__))
T, N, CLIP = 12, 5, np.float32(100.0)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sensor") / "libsensor_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "sensor_emul.cpp")])
    L = C.CDLL(out)
    L.sensor_emul.argtypes = [C.c_void_p] * 4 + [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3
    return L


def _run(L, y, done, d_imu, d_joint, bias, ring=None, count=None):
    t, n, _ = y.shape
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    delay = np.ascontiguousarray(np.stack([d_imu, d_joint], axis=1).astype(np.int32))
    out = np.full_like(y, 7.0)
    ring = np.zeros((n, 4, sn.NOBS), np.float32) if ring is None else ring
    count = np.zeros(n, np.uint32) if count is None else count
    d8 = np.ascontiguousarray(done.astype(np.uint8))
    assert L.sensor_emul(p(y), p(d8), p(delay), p(np.ascontiguousarray(bias)), C.c_float(CLIP), t, n, p(out), p(ring), p(count)) == 0
    return out, ring, count


def _inputs(seed=1):
    r = np.random.default_rng(seed)
    y = r.normal(size=(T, N, sn.NOBS)).astype(np.float32)
    y[2, 1, 5], y[7, 3, 40], y[9, 0, 13], y[4, 2, 50] = 180.0, -300.0, 99.9, 120.0      # beyond the clamp in a few cells (one a pass-through column)
    y[3, :, 10], y[5, 2, 60], y[6, 4, 0] = -0.0, -0.0, -0.0
    done = np.zeros((T, N), bool)
    done[0, 0] = True                                  # a done at step 0
    done[4, 1] = done[5, 1] = True                     # two dones on consecutive steps
    done[8, 3] = done[10, 4] = done[11, 0] = True      # env 2 has none
    return y, done


def test_every_delay_pair_against_the_restatement(emul):
    y, done = _inputs()
    r = np.random.default_rng(2)
    pairs = [(a, b) for a in range(4) for b in range(4)]
    clamped = 0
    for k in range(0, 16, N):                          # five envs at a time, all 16 pairs of 0..3 (the last round repeats some)
        chunk = (pairs + pairs)[k:k + N]
        d_imu, d_joint = np.array([p[0] for p in chunk]), np.array([p[1] for p in chunk])
        bias = r.uniform(-0.5, 0.5, (N, sn.NOBS)).astype(np.float32)
        bias[:, sn.PASS] = 0.0
        bias[1, 5], bias[3, 40] = 30.0, -60.0          # a sum beyond the clamp, from both sides
        got, ring, count = _run(emul, y, done, d_imu, d_joint, bias)
        want, want_count = sn.sensed(y, done, d_imu, d_joint, bias, CLIP)
        np.testing.assert_array_equal(got.view(np.uint32)[..., sn.PASS], y.view(np.uint32)[..., sn.PASS])      # bit-identical, -0.0 included
        assert np.array_equal(got, want), (chunk, np.argwhere(got != want)[:5])
        np.testing.assert_array_equal(got.view(np.uint32)[..., np.r_[sn.IMU, sn.JOINT]], want.view(np.uint32)[..., np.r_[sn.IMU, sn.JOINT]])
        np.testing.assert_array_equal(count, want_count)
        clamped += int((np.abs(got[..., np.r_[sn.IMU, sn.JOINT]]) == CLIP).sum())
        # the ring holds the last four true rows where the env's count says they lie
        for e in range(N):
            pushed = T - int(want_count[e])            # steps before the env's last clear
            for j in range(min(int(count[e]), 4)):
                s = T - 1 - j
                np.testing.assert_array_equal(ring[e, (s - pushed) % 4], y[s, e])
    assert clamped > 0                                 # the clamp was met


def test_zero_model_is_the_true_row_and_a_split_sequence_continues(emul):
    y, done = _inputs(3)
    z = np.zeros(N, np.int32)
    got, _, _ = _run(emul, y, done, z, z, np.zeros((N, sn.NOBS), np.float32))
    assert np.array_equal(got, np.where(np.isin(np.arange(sn.NOBS), sn.PASS), y, np.clip(y, -CLIP, CLIP)))      # the step has clipped already: then the row itself
    d_imu, d_joint, bias = sn.model(N, 4)
    whole, ring, count = _run(emul, y, done, d_imu, d_joint, bias)
    a, r1, c1 = _run(emul, y[:5], done[:5], d_imu, d_joint, bias)
    b, r2, c2 = _run(emul, y[5:], done[5:], d_imu, d_joint, bias, r1, c1)
    assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(r2, ring) and np.array_equal(c2, count)
    assert np.array_equal(whole, sn.sensed(y, done, d_imu, d_joint, bias, CLIP)[0])
