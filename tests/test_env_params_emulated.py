"""Per-env friction and servo gains (nm::Args::envp) in the host emulation of the device source (tests/emul/nm_emul.cpp):
the fp64 emulation of a batch that mixes the four parameter sets over its envs against the fp64 fixture of the oracle's rows
(tests/golden/make_envparam_goldens.py), mixed batches against uniform ones bit for bit, identity values against no rows at all, and
the stand-alone sanitizer build of the shim. The fixture's states are teacher-forced: env e of the mixed batch starts every step from the
recorded state of env e of ITS set's trajectory."""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden

POPS = ("drop", "stand", "belly")


@pytest.fixture(scope="module")
def G():
    return load_golden("env_params.npz")


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.ROWS)
    return em


def set_of(n, shift=0):
    """Parameter set of env e: neighbours in a wave (2w, 2w + 1) always hold different sets, and every set meets every slot."""
    e = np.arange(n)
    return (e + e // 4 + shift) % 4


def load_step(env, g, pop, t, sets):
    """Start state of step t: env e takes env e % 8 of the trajectory of set sets[e]."""
    n = len(sets)
    ev = np.arange(n) % 8
    pick = lambda k: g[f"{pop}_{k}"][sets, t, ev]
    env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
    env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
    env.eplen[:] = pick("ep_len")
    return g[f"{pop}_actions"][sets, t, ev], g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64)


def errors(env, g, pop, t, sets, obs, rew, done):
    ev = np.arange(len(sets)) % 8
    oerr = np.abs(obs.astype(np.float64) - g[f"{pop}_obs"][sets, t, ev]).max(axis=1)
    rerr = np.abs(rew.astype(np.float64) - g[f"{pop}_rew"][sets, t, ev])
    serr = max(np.abs(env.get("qpos") - g[f"{pop}_qpos"][sets, t + 1, ev]).max(), np.abs(env.get("qvel") - g[f"{pop}_qvel"][sets, t + 1, ev]).max())
    return oerr, rerr, serr, int((done != g[f"{pop}_done"][sets, t, ev]).sum())


def run_forced(emul, g, pop, sets, double, rows="sets", steps=None, envs_per_wave=2):
    """Teacher-forced single steps of one batch; returns per-step (obs, rew, qpos, qvel), the error figures, and the debug rows."""
    n = len(sets)
    env = emul.EmulRows(n, double=double, seed=5, envs_per_wave=envs_per_wave)
    if isinstance(rows, str):        # "sets": every env its own set
        env.set_env_params(g["sets"][sets])
    elif rows is not None:
        env.set_env_params(rows)
    out, oerrs, serr, ntog, nbig, flags = [], [], 0.0, 0, 0, 0
    T = g[f"{pop}_actions"].shape[1] if steps is None else steps
    for t in range(T):
        a, cu = load_step(env, g, pop, t, sets)
        obs, rew, done, _ = env.step(a, cmd_u=cu, want_dbg=True)
        oe, re_, se, fl = errors(env, g, pop, t, sets, obs, rew, done)
        flags += fl
        oerrs.append(np.maximum(oe, re_))
        serr = max(serr, se)
        out.append((obs.copy(), rew.copy(), env.get("qpos"), env.get("qvel")))
        ntog += int(env.dbg[0::2, emul.DBG_NTOG].sum())
        nbig += int((env.dbg[:, emul.DBG_NCON] > 16).sum())      # ncon > kMaxCon (16) IS the dispatch to stage_constraint_big (nm_core.h stage_constraint)
    return out, (np.stack(oerrs), flags), serr, ntog, nbig


def same(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("pop", POPS)
def test_fp64_emulation_of_a_mixed_batch_matches_the_variant_oracles(G, emul, pop, envs_per_wave):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8). Two envs per wave is the fp32
    kernel's layout, one env per wave the fp64 kernel's (its own load stage)."""
    sets = set_of(16)
    tog0 = emul.lib(emul.ROWS).emu_together_count()
    _, (err, flags), serr, ntog, nbig = run_forced(emul, G, pop, sets, double=True, envs_per_wave=envs_per_wave)
    assert flags == 0
    print(f"{pop}: max obs/reward error {err.max():.2e}, max state error {serr:.2e}, two-env passes {ntog}, env-steps above 16 contacts {nbig}")
    assert err.max() < 1e-6 and serr < 1e-8, (err.max(), serr)
    if pop == "stand" and envs_per_wave == 2:      # both envs of a wave in ONE constraint pass, with different friction in its halves
        assert ntog > 0 and emul.lib(emul.ROWS).emu_together_count() > tog0
        assert (G["sets"][sets[0::2], 0] != G["sets"][sets[1::2], 0]).all()
    if pop == "belly":      # the matrix-free layout ran
        assert nbig >= 4


@pytest.mark.parametrize("pop", POPS)
def test_fp32_mixed_batch_equals_uniform_batches_bit_for_bit(G, emul, pop):
    """Every env is independent: env e of the mixed batch must equal env e of the batch in which EVERY env holds e's set - same states,
    same actions, so the only thing that differs between the two runs is what the wave's other env carries."""
    n, steps = 8, (4 if pop != "belly" else G["belly_actions"].shape[1])      # belly: every step, so that the steps above 16 contacts are in
    sets = set_of(n)
    mixed, (err, flags), _, ntog, nbig = run_forced(emul, G, pop, sets, double=False, steps=steps)
    assert flags == 0
    # first confirmed here, on the CPU: the fixture's states keep the fp32 arithmetic inside the bounds the GPU test asserts
    print(f"{pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4
    for k in range(4):
        rows = np.repeat(G["sets"][k][None], n, axis=0)
        uni, _, _, _, _ = run_forced(emul, G, pop, sets, double=False, rows=rows, steps=steps)
        m = sets == k
        assert m.any()
        for (o1, r1, q1, v1), (o2, r2, q2, v2) in zip(mixed, uni):
            np.testing.assert_array_equal(o1[m], o2[m]); np.testing.assert_array_equal(r1[m], r2[m])
            np.testing.assert_array_equal(q1[m], q2[m]); np.testing.assert_array_equal(v1[m], v2[m])
    if pop == "stand":
        assert ntog > 0
    if pop == "belly":
        assert nbig >= 1


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_identity_values_equal_no_rows_bit_for_bit(G, emul, double):
    sets = np.zeros(8, int)             # set 0 is (1.0, 20.0, 0.8): the model's own values
    np.testing.assert_array_equal(G["sets"][0], [1.0, 20.0, 0.8])
    for pop in POPS:
        off, _, _, _, _ = run_forced(emul, G, pop, sets, double=double, rows=None, steps=3)
        on, _, _, _, _ = run_forced(emul, G, pop, sets, double=double, rows="sets", steps=3)
        same(off, on)


def test_parameters_change_the_physics(G, emul):
    """The rows are not ignored: another friction, stiffness or damping moves a standing robot's next state."""
    sets = np.zeros(8, int)

    def qvel_after(rows):
        env = emul.EmulRows(8, double=True, seed=5)
        env.set_env_params(rows)
        a, cu = load_step(env, G, "stand", 0, sets)
        env.step(a, cmd_u=cu)
        return env.get("qvel")

    base = qvel_after(None)
    for col, val in ((0, 0.4), (1, 14.0), (2, 1.1)):
        rows = np.repeat(G["sets"][0][None], 8, axis=0)
        rows[:, col] = val
        assert np.abs(qvel_after(rows) - base).max() > 1e-9, col


def test_standalone_sanitizer_build_of_the_shim_runs_clean(G, emul, tmp_path):
    """The shim as a program of its own (its own main, nothing loaded into Python) under AddressSanitizer and UBSan: one mixed-batch step
    of each population from the fixture's states, fp32 and fp64; exit status 0 = no report, every value finite, the two-env pass and the
    matrix-free layout both taken."""
    sets, ev, parts = set_of(8), np.arange(8), []
    for pop in POPS:
        t = int(np.argmax((G[f"{pop}_ncon"] > 16).sum(axis=(0, 2)))) if pop == "belly" else 0
        for k in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "actions"):
            parts.append(np.asarray(G[f"{pop}_{k}"][sets, t, ev], np.float64).ravel())
    states = tmp_path / "states.bin"
    np.concatenate(parts).tofile(states)
    exe = emul.build_program(str(tmp_path / "nm_emul_asan"), (1,), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], opt="-O0")
    r = subprocess.run([exe, "envp", str(states)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "fp32" in r.stdout and "fp64" in r.stdout
