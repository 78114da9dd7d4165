"""Per-env base payloads (body rows, level 2 of the step) in the host emulation of the device source (tests/emul/nm_emul.cpp):
the fp64 emulation of a batch that mixes the four payload sets over its envs against the fp64 fixture of the variant oracles
(tests/golden/make_payload_goldens.py: the unchanged oracle compiled against the header of the recompiled model), mixed batches against
uniform ones bit for bit, the default row against no rows at all, and the stand-alone sanitizer build of the shim. The body rows come
from nightmare_rl_amd.model.payload.payload_rows, the batched host derivation. The fixture's states are teacher-forced: env e of the
mixed batch starts every step from the recorded state of env e of ITS set's trajectory."""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden

POPS = ("drop", "stand", "belly")


@pytest.fixture(scope="module")
def G():
    return load_golden("payload.npz")


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.ROWS)
    return em


@pytest.fixture(scope="module")
def ROWS(G):
    from nightmare_rl_amd.model import payload
    return payload.payload_rows(G["sets"][:, 0], G["sets"][:, 1:])


def set_of(n, shift=0):
    """Payload set of env e: neighbours in a wave (2w, 2w + 1) always hold different sets, and every set meets every slot."""
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


def run_forced(emul, g, pop, sets, double, rows, steps=None, envs_per_wave=2, envp=None):
    """Teacher-forced single steps of one batch; returns per-step (obs, rew, qpos, qvel), the error figures, and the debug rows."""
    n = len(sets)
    env = emul.EmulRows(n, double=double, seed=5, envs_per_wave=envs_per_wave)
    if envp is not None:
        env.set_env_params(envp)
    if isinstance(rows, str):        # "default": the model's own row in every env, set explicitly
        env.set_body_params(np.repeat(env.default_row()[None], n, axis=0))
    elif rows is not None:
        env.set_body_params(rows)
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
def test_fp64_emulation_of_a_mixed_batch_matches_the_variant_oracles(G, ROWS, emul, pop, envs_per_wave):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8). Two envs per wave is the fp32
    kernel's layout, one env per wave the fp64 kernel's (its own load stage)."""
    sets = set_of(16)
    tog0 = emul.lib(emul.ROWS).emu_together_count()
    _, (err, flags), serr, ntog, nbig = run_forced(emul, G, pop, sets, double=True, rows=ROWS[sets], envs_per_wave=envs_per_wave)
    assert flags == 0
    print(f"{pop}: max obs/reward error {err.max():.2e}, max state error {serr:.2e}, two-env passes {ntog}, env-steps above 16 contacts {nbig}")
    assert err.max() < 1e-6 and serr < 1e-8, (err.max(), serr)
    if pop == "stand" and envs_per_wave == 2:      # both envs of a wave in ONE constraint pass, with different payloads in its halves
        assert ntog > 0 and emul.lib(emul.ROWS).emu_together_count() > tog0
        assert (sets[0::2] != sets[1::2]).all() and len({tuple(r) for r in ROWS}) == 4
    if pop == "belly":      # the matrix-free layout ran
        assert nbig >= 4


@pytest.mark.parametrize("pop", POPS)
def test_fp32_mixed_batch_equals_uniform_batches_bit_for_bit(G, ROWS, emul, pop):
    """Every env is independent: env e of the mixed batch must equal env e of the batch in which EVERY env holds e's payload - same
    states, same actions, so the only thing that differs between the two runs is what the wave's other env carries."""
    n, steps = 8, (4 if pop != "belly" else G["belly_actions"].shape[1])      # belly: every step, so that the steps above 16 contacts are in
    sets = set_of(n)
    mixed, (err, flags), _, ntog, nbig = run_forced(emul, G, pop, sets, double=False, rows=ROWS[sets], steps=steps)
    assert flags == 0
    # first confirmed here, on the CPU: the fixture's states keep the fp32 arithmetic inside the bounds the GPU test asserts
    print(f"{pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4
    for k in range(4):
        uni, _, _, _, _ = run_forced(emul, G, pop, sets, double=False, rows=np.repeat(ROWS[k][None], n, axis=0), steps=steps)
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
def test_default_rows_equal_no_rows_bit_for_bit(G, emul, double):
    """The model's own row set explicitly in every env (level 2 of the step, default friction / gain rows) against no rows at all
    (level 0): the expressions kept their shape, so the bits are the same."""
    sets = np.zeros(8, int)
    np.testing.assert_array_equal(G["sets"][0], [0.0, 0.0, 0.0, 0.0])
    for pop in POPS:
        steps = 3 if pop != "belly" else G["belly_actions"].shape[1]
        off, _, _, _, _ = run_forced(emul, G, pop, sets, double=double, rows=None, steps=steps)
        on, _, _, ntog, nbig = run_forced(emul, G, pop, sets, double=double, rows="default", steps=steps)
        same(off, on)
        if pop == "belly":
            assert nbig >= 1
        if pop == "stand" and not double:
            assert ntog > 0


def test_default_row_is_the_committed_model(G, ROWS, emul):
    """payload_rows(0) and the row the C side takes from its Tables agree (fp64: to rounding of the sums)."""
    env = emul.EmulRows(2, double=True)
    np.testing.assert_allclose(env.default_row(), ROWS[0], rtol=1e-12, atol=1e-17)
    np.testing.assert_allclose(G["rows"], ROWS, rtol=1e-9, atol=1e-15)


def test_payload_with_friction_and_gains_equals_the_uniform_runs(G, ROWS, emul):
    """Both kinds of rows set: env e equals the run in which every env holds e's payload AND e's friction / gains (fp32, bit for bit)."""
    n, pop, steps = 8, "stand", 3
    sets = set_of(n)
    envp_sets = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])
    esets = set_of(n, shift=1)
    mixed, _, _, ntog, _ = run_forced(emul, G, pop, sets, double=False, rows=ROWS[sets], steps=steps, envp=envp_sets[esets])
    assert ntog > 0
    for e in range(n):
        uni, _, _, _, _ = run_forced(emul, G, pop, sets, double=False, rows=np.repeat(ROWS[sets[e]][None], n, axis=0), steps=steps,
                                     envp=np.repeat(envp_sets[esets[e]][None], n, axis=0))
        for a, b in zip(mixed, uni):
            for u, v in zip(a, b):
                np.testing.assert_array_equal(u[e], v[e])
    # payload alone (the shim fills default friction / gain rows, as the host does) = the same payload with those rows set explicitly
    alone, _, _, _, _ = run_forced(emul, G, pop, sets, double=False, rows=ROWS[sets], steps=steps)
    both, _, _, _, _ = run_forced(emul, G, pop, sets, double=False, rows=ROWS[sets], steps=steps, envp=np.repeat(envp_sets[0][None], n, axis=0))
    same(alone, both)


def test_payload_changes_the_physics(G, ROWS, emul):
    """The rows are not ignored: each word group moves a standing robot's next state."""
    sets = np.zeros(8, int)

    def qvel_after(rows):
        env = emul.EmulRows(8, double=True, seed=5)
        env.set_body_params(rows)
        a, cu = load_step(env, G, "stand", 0, sets)
        env.step(a, cmd_u=cu)
        return env.get("qvel")

    base = qvel_after(None)
    for lo, hi in ((0, 3), (3, 9), (9, 10), (11, 18)):      # ipos, inertia, mass, invweight0 (total_mass and pgs_scale do not reach qvel in one quiet step)
        rows = np.repeat(ROWS[0][None], 8, axis=0)
        rows[:, lo:hi] = ROWS[3][lo:hi]
        assert np.abs(qvel_after(rows) - base).max() > 1e-9, (lo, hi)


def test_standalone_sanitizer_build_of_the_shim_runs_clean(G, ROWS, emul, tmp_path):
    """The shim as a program of its own (its own main, nothing loaded into Python) under AddressSanitizer and UBSan: one mixed-batch step
    of each population from the fixture's states, fp32 and fp64; exit status 0 = no report, every value finite, the two-env pass and the
    matrix-free layout both taken."""
    sets, ev, parts = set_of(8), np.arange(8), [np.asarray(ROWS, np.float64).ravel()]
    for pop in POPS:
        t = int(np.argmax((G[f"{pop}_ncon"] > 16).sum(axis=(0, 2)))) if pop == "belly" else 0
        for k in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "actions"):
            parts.append(np.asarray(G[f"{pop}_{k}"][sets, t, ev], np.float64).ravel())
    states = tmp_path / "states.bin"
    np.concatenate(parts).tofile(states)
    exe = emul.build_program(str(tmp_path / "nm_emul_asan"), (2,), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], opt="-O0")
    r = subprocess.run([exe, "payload", str(states)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "fp32" in r.stdout and "fp64" in r.stdout
