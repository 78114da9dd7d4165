"""Per-env actuation latency (nm_set_action_latency, level 3 of the step) in the host emulation of the device source
(tests/emul/nm_emul.cpp): the fp64 emulation of the fixture's mixed batch - delays 0..6 and 0 over eight envs - against the fp64
fixture of the oracle's rows (tests/golden/make_latency_goldens.py), delay 0 against no delays at all and the mixed batch against the
seven uniform ones bit for bit, and the stand-alone sanitizer build of the shim. The fixture's states are teacher-forced: every step
starts from the recorded state AND the recorded action history."""
import subprocess

import numpy as np
import pytest

from conftest import load_golden

POPS = ("drop", "stand")


@pytest.fixture(scope="module")
def G():
    return load_golden("latency.npz")


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.ROWS)
    return em


def load_step(env, g, pop, t, n=8):
    """Start state of step t; env e takes env e % 8 of the fixture (n = 16: the batch twice)."""
    ev = np.arange(n) % 8
    pick = lambda k: g[f"{pop}_{k}"][t, ev]
    env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
    env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
    env.eplen[:] = pick("ep_len")
    env.history[:] = pick("hist")
    return pick("actions"), pick("cmd_u").astype(np.float64)


def run_forced(emul, g, pop, delays, double, steps=None, envs_per_wave=2):
    """Teacher-forced single steps of one batch under `delays` ([n], or None = the launch carries no rows); returns per-step
    (obs, rew, qpos, qvel, qwarm, history), the error figures against the fixture (meaningful where delays are the fixture's), the
    number of two-env constraint passes."""
    n = 8 if delays is None else len(delays)
    ev = np.arange(n) % 8
    env = emul.EmulRows(n, double=double, seed=5, envs_per_wave=envs_per_wave)
    env.set_action_latency(delays)
    out, oerrs, serr, ntog, flags = [], [], 0.0, 0, 0
    T = g[f"{pop}_actions"].shape[0] if steps is None else steps
    for t in range(T):
        a, cu = load_step(env, g, pop, t, n)
        obs, rew, done, _ = env.step(a, cmd_u=cu, want_dbg=True)
        oe = np.abs(obs.astype(np.float64) - g[f"{pop}_obs"][t, ev]).max(axis=1)
        re_ = np.abs(rew.astype(np.float64) - g[f"{pop}_rew"][t, ev])
        serr = max(serr, np.abs(env.get("qpos") - g[f"{pop}_qpos"][t + 1, ev]).max(), np.abs(env.get("qvel") - g[f"{pop}_qvel"][t + 1, ev]).max())
        flags += int((done != g[f"{pop}_done"][t, ev]).sum())
        oerrs.append(np.maximum(oe, re_))
        out.append((obs.copy(), rew.copy(), env.get("qpos"), env.get("qvel"), env.get("qwarm"), env.history.copy()))
        ntog += int(env.dbg[0::2, emul.DBG_NTOG].sum())
    return out, (np.stack(oerrs), flags), serr, ntog


def same(a, b, m=slice(None)):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u[m], v[m])


@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("pop", POPS)
def test_fp64_emulation_of_the_mixed_batch_matches_the_patched_oracle(G, emul, pop, envs_per_wave):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8). Two envs per wave is the fp32
    kernel's layout, one env per wave the fp64 kernel's (its own load stage). 16 envs: the fixture's batch twice."""
    delays = np.tile(G["delays"], 2)
    out, (err, flags), serr, ntog = run_forced(emul, G, pop, delays, double=True, envs_per_wave=envs_per_wave)
    assert flags == 0
    print(f"{pop}: max obs/reward error {err.max():.2e}, max state error {serr:.2e}, two-env passes {ntog}")
    assert err.max() < 1e-6 and serr < 1e-8, (err.max(), serr)
    for t, o in enumerate(out):      # the history after the step is the fixture's: shifted, this step's scaled and clipped action in front
        np.testing.assert_array_equal(o[5], np.tile(G[f"{pop}_hist"][t + 1], (2, 1, 1)))
    # observation slots 48..65 keep this step's own action whatever the delay
    np.testing.assert_array_equal(out[0][0][:8, 48:66], G[f"{pop}_hist"][1][:, 0])
    if pop == "stand" and envs_per_wave == 2:      # both envs of a wave in ONE constraint pass, switching at different substeps
        assert ntog > 0
        r = G["delays"] % 2
        assert (r[0:6:2] != r[1:6:2]).all()      # waves (0,1), (2,3), (4,5); the last wave holds delays 6 and 0: both r = 0


@pytest.mark.parametrize("pop", POPS)
def test_fp32_emulation_stays_inside_the_fp32_bounds(G, emul, pop):
    """First confirmed here, on the CPU: the fixture's states keep the fp32 arithmetic inside the bounds the GPU test asserts."""
    _, (err, flags), _, _ = run_forced(emul, G, pop, G["delays"], double=False)
    assert flags == 0
    print(f"{pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_delay_zero_equals_no_delays_bit_for_bit(G, emul, double):
    for pop in POPS:
        off, _, _, _ = run_forced(emul, G, pop, None, double=double, steps=3)
        on, _, _, _ = run_forced(emul, G, pop, np.zeros(8, np.int32), double=double, steps=3)
        for x, y in zip(off, on):      # (the launch without rows never touches the history: compare everything else)
            for u, v in zip(x[:5], y[:5]):
                np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("pop", POPS)
def test_mixed_batch_equals_uniform_batches_bit_for_bit(G, emul, pop, double):
    """Every env is independent: env e of the mixed batch must equal env e of the batch in which EVERY env holds e's delay - same states,
    same histories, same actions, so the only thing that differs between the two runs is when the wave's other env switches."""
    delays, steps = G["delays"], 4
    mixed, _, _, ntog = run_forced(emul, G, pop, delays, double=double, steps=steps)
    for d in range(7):
        uni, _, _, _ = run_forced(emul, G, pop, np.full(8, d, np.int32), double=double, steps=steps)
        m = delays == d
        assert m.any()
        same(mixed, uni, m)
    if pop == "stand" and not double:
        assert ntog > 0


def test_delays_change_the_physics(G, emul):
    """The delays are not ignored: every delayed env's next state differs from the undelayed step's, an undelayed env's does not."""
    def qvel_after(delays):
        env = emul.EmulRows(8, double=True, seed=5)
        env.set_action_latency(delays)
        a, cu = load_step(env, G, "stand", 0)
        env.step(a, cmd_u=cu)
        return env.get("qvel")

    diff = np.abs(qvel_after(G["delays"]) - qvel_after(None)).max(axis=1)
    assert (diff[G["delays"] > 0] > 1e-9).all() and (diff[G["delays"] == 0] == 0).all(), diff


def test_physics_only_launch_ignores_latency(G, emul):
    def after(delays):
        env = emul.EmulRows(8, double=False, seed=5)
        env.set_action_latency(delays)
        a, _ = load_step(env, G, "stand", 0)
        h0 = env.history.copy()
        env.step(a, physics_only=True)
        np.testing.assert_array_equal(env.history, h0)
        return env.get("qpos"), env.get("qvel")

    for u, v in zip(after(G["delays"]), after(None)):
        np.testing.assert_array_equal(u, v)


def test_standalone_sanitizer_build_of_the_shim_runs_clean(G, emul, tmp_path):
    """The shim as a program of its own (its own main, nothing loaded into Python) under AddressSanitizer and UBSan: one mixed-batch step
    of each population from the fixture's states and histories, fp32 and fp64; exit status 0 = no report, every value finite, the two-env
    pass taken, every history shifted."""
    parts = []
    for pop in POPS:
        for k in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "actions", "hist"):
            parts.append(np.asarray(G[f"{pop}_{k}"][0], np.float64).ravel())
    states = tmp_path / "states.bin"
    np.concatenate(parts).tofile(states)
    exe = emul.build_program(str(tmp_path / "nm_emul_asan"), (3,), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], opt="-O0")
    r = subprocess.run([exe, "latency", str(states)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "fp32" in r.stdout and "fp64" in r.stdout
