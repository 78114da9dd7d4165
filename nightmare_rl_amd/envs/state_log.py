"""StateLog: the host side of `cfg.viewer.record_states` (reference envs/nightmare_v3_env.py:261-272; reader open_custom_play.py:50-66).

Upstream, per step: `if reset_buf[0]: pickle.dump(recorded_states, <log_dir>/<int(time.time())>.pkl); recorded_states = []`, THEN
`recorded_states.append((data[0].time, qpos, qvel, act))` with the state as it is after the physics and before reset_idx. So the record of
the step in which env 0 resets is the FIRST entry of the next file. This class owns that order, the `data.time` bookkeeping (MuJoCo's
mj_resetData restarts the clock when a bad state is detected inside the step) and the file naming; it has no device code and no
dependency on one: the env feeds it one row after a step() or K rows after a K-step launch (nm_get_state_log), with the same result.

File names: upstream's `<int(time.time())>.pkl`. A K-step launch can dump several files within one second (upstream would overwrite the
earlier one), and open_custom_play.py:23 plays them in `sorted()` order, so a taken name gets a suffix that sorts after it and in write
order: `<sec>.pkl`, `<sec>_0001.pkl`, `<sec>_0002.pkl`, ... ('.' < '_' in ASCII, the counter is zero padded). The same holds for names
another StateLog or an earlier run left in the directory.
"""
import os
import pickle
import time

import numpy as np

NQ, NV = 25, 24
ROW = NQ + NV + 1          # qpos | qvel | bad-state resets inside the step (nm_get_state_record / nm_get_state_log)


class StateLog:
    def __init__(self, log_dir, sim_dt, clock=time.time):
        """sim_dt: seconds of simulated time per env step (model timestep x decimation); clock: what names the files (tests inject one)."""
        self.log_dir = log_dir
        self.sim_dt = float(sim_dt)
        self.clock = clock
        self.records = []          # upstream's self.recorded_states: what has been logged since the last dump
        self.time = 0.0            # upstream's data[0].time
        self.files = []            # paths written, in write order

    def _path(self):
        sec = int(self.clock())
        p = os.path.join(self.log_dir, f"{sec}.pkl")
        k = 0
        while os.path.exists(p):
            k += 1
            p = os.path.join(self.log_dir, f"{sec}_{k:04d}.pkl")
        return p

    def dump(self):
        os.makedirs(self.log_dir, exist_ok=True)
        p = self._path()
        with open(p, "wb") as f:
            pickle.dump(self.records, f)
        self.files.append(p)
        self.records = []
        return p

    def add(self, qpos, qvel, bad_state_resets, done):
        """One step: `done` = the logged env's reset flag of this step (reference :263 tests reset_buf[0] before it appends)."""
        if done:
            self.dump()
        self.time = self.sim_dt if bad_state_resets else self.time + self.sim_dt     # mj_resetData restarts data.time
        self.records.append((self.time, np.array(qpos, np.float64), np.array(qvel, np.float64), np.zeros(0)))   # no actuator state: act is empty

    def add_rows(self, rows, dones):
        """K steps at once: rows [K, 50] = qpos 25 | qvel 24 | bad-state resets (nm_get_state_log), dones [K] the logged env's reset flags."""
        rows = np.asarray(rows, np.float64).reshape(-1, ROW)
        dones = np.asarray(dones).reshape(-1)
        if rows.shape[0] != dones.shape[0]:
            raise ValueError("StateLog.add_rows: one done flag per row")
        for r, d in zip(rows, dones):
            self.add(r[:NQ], r[NQ:NQ + NV], int(r[NQ + NV]), bool(d))
