"""The sensor model (observation latency and bias; include/nightmare_hip.h nm_set_sensor) restated in numpy from its three rules, for the
tests that hold the header's sensor_apply (host emulation) and the device paths against it. Not a transliteration of csrc/nm_sensor.h: there
is no ring and no counter here - a reading looks back into the list of true observations, but never behind the last clear."""
import numpy as np

NOBS = 66
IMU = np.arange(0, 9)                                            # base lin vel, base ang vel, projected gravity
JOINT = np.arange(12, 48)                                        # dof_pos, dof_vel
PASS = np.concatenate([np.arange(9, 12), np.arange(48, 66)])    # commands, previous actions
KIND_COLS = {"lin_vel": np.arange(0, 3), "ang_vel": np.arange(3, 6), "gravity": np.arange(6, 9), "dof_pos": np.arange(12, 30),
             "dof_vel": np.arange(30, 48)}
SENSOR_KEY = 0x53454E534F       # nm_sensor.h kSensorKey ("SENSO")


def sensed(y, done, d_imu, d_joint, bias, clip):
    """y [T, N, 66] float32 true observations, done [T, N] bool, d_imu / d_joint [N] whole steps, bias [N, 66] float32, clip a float32.
    Returns (sensed [T, N, 66] float32, count [N]): the history is clear before step 0; count is what is left in it after step T - 1."""
    y, bias, clip = np.asarray(y, np.float32), np.asarray(bias, np.float32), np.float32(clip)
    T, N, _ = y.shape
    out = y.copy()                                               # the pass-through columns are the step's own words
    count = np.zeros(N, np.uint32)
    for e in range(N):
        first = 0                                                # the oldest step a reading may reach: the one after the last clear
        for s in range(T):
            for cols, d in ((IMU, int(d_imu[e])), (JOINT, int(d_joint[e]))):
                src = max(s - d, first)
                v = (y[src, e, cols] + bias[e, cols]).astype(np.float32)       # one float32 add
                out[s, e, cols] = np.minimum(np.maximum(v, -clip), clip)
            if done[s, e]:
                first = s + 1                                    # after the read: the done step's own reading was delayed like any other
        count[e] = T - first
    return out, count


def model(N, seed=0, big=True):
    """(d_imu, d_joint, bias): delays that run through 0..3 in both groups across the envs (in opposite order, so that N = 5 holds every value
    in both), random bias rows with zeros in the pass-through columns and - `big` - one offset that drives a column into the clamp."""
    r = np.random.default_rng(seed)
    d_imu, d_joint = (np.arange(N) % 4).astype(np.int32), ((3 - np.arange(N)) % 4).astype(np.int32)
    bias = r.uniform(-0.25, 0.25, (N, NOBS)).astype(np.float32)
    bias[:, PASS] = 0.0
    if big:
        bias[0, 4], bias[N - 1, 20] = 250.0, -250.0
    return d_imu, d_joint, bias
