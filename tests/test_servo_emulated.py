"""The servo target model (nm_set_servo, level 5 of the step) in the host emulation of the device source (tests/emul/nm_emul.cpp,
levels 0 and 5 only): the fp64 emulation of the fixture's mixed batch against the fp64 fixture of the oracle's rows
(tests/golden/make_servo_goldens.py), alone (S) and behind the delays 0..6, 0 (SL), teacher-forced and free-running, with the limited
targets after every step; the fp32 emulation inside the project's fp32 bounds; default rows at level 5 against level 0 under ==; the mixed
batch against the uniform ones bit for bit; a physics-only launch; and the stand-alone sanitizer build of the shim."""
import subprocess

import numpy as np
import pytest

from conftest import load_golden

POPS = ("drop", "stand")
RECS = ("S", "SL")


@pytest.fixture(scope="module")
def G():
    return load_golden("servo.npz")


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.SERVO)
    return em


def delays_of(g, rec):
    return g["delays"] if rec == "SL" else None


def load_step(env, g, rec, pop, t, state=True):
    """Start state of step t of a recording (state False: the step's inputs only - a free-running env keeps its own state)."""
    pick = lambda k: g[f"{rec}_{pop}_{k}"][t]
    if state:
        env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
        env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
        env.eplen[:] = pick("ep_len")
        env.history[:] = pick("hist")
        env.set_servo_state(pick("lim"))
    return pick("actions"), pick("cmd_u").astype(np.float64)


def run(emul, g, rec, pop, rate, d_gain, double, steps=None, envs_per_wave=2, forced=True, delays="rec"):
    """Single steps of the fixture's batch under (rate, d_gain) ([8] each, or both None = the launch carries no rows) and the recording's
    delays; teacher-forced (every step from the recorded state, history and limited targets) or free-running from the first. Returns
    per-step (obs, rew, qpos, qvel, qwarm, limited targets) and the error figures against the recording."""
    env = emul.EmulServo(8, double=double, seed=5, envs_per_wave=envs_per_wave)
    env.set_servo(rate, d_gain)
    d = delays_of(g, rec) if isinstance(delays, str) else delays
    if d is not None:
        env.set_action_latency(d)
    out, oerrs, serr, lerr, flags = [], [], 0.0, 0.0, 0
    T = g[f"{rec}_{pop}_actions"].shape[0] if steps is None else steps
    for t in range(T):
        a, cu = load_step(env, g, rec, pop, t, state=forced or t == 0)
        obs, rew, done, _ = env.step(a, cmd_u=cu)
        oe = np.abs(obs.astype(np.float64) - g[f"{rec}_{pop}_obs"][t]).max(axis=1)
        re_ = np.abs(rew.astype(np.float64) - g[f"{rec}_{pop}_rew"][t])
        serr = max(serr, np.abs(env.get("qpos") - g[f"{rec}_{pop}_qpos"][t + 1]).max(), np.abs(env.get("qvel") - g[f"{rec}_{pop}_qvel"][t + 1]).max())
        lerr = max(lerr, np.abs(env.servo_state() - g[f"{rec}_{pop}_lim"][t + 1]).max())
        flags += int((done != g[f"{rec}_{pop}_done"][t]).sum())
        oerrs.append(np.maximum(oe, re_))
        out.append((obs.copy(), rew.copy(), env.get("qpos"), env.get("qvel"), env.get("qwarm"), env.servo_state()))
    return out, (np.stack(oerrs), flags), serr, lerr


def same(a, b, m=slice(None), upto=None):
    for x, y in zip(a, b):
        for u, v in zip(x[:upto], y[:upto]):
            np.testing.assert_array_equal(u[m], v[m])


def test_layout_and_level(emul):
    for n in (1, 7, 8):
        for double in (False, True):
            env = emul.EmulServo(n, double=double)
            assert env.layout_agrees(), n
            assert env.level() == 0 and env.level(True) == 0
            rate, d_gain = env.servo()
            assert np.isinf(rate).all() and (d_gain == 0).all()      # the region holds the defaults while the kind is off
            env.set_servo(0.05, 0.1)
            assert env.level() == 5 and env.level(True) == 5
            env.set_servo()
            assert env.level() == 0 and np.isinf(env.servo()[0]).all()
    env = emul.EmulServo(4)
    for bad in ((0.0, 0.0), (-1.0, 0.0), (np.nan, 0.0), (0.1, -0.1), (0.1, np.inf), (0.1, np.nan)):
        with pytest.raises(ValueError):
            env.set_servo(*bad)
        assert env.level() == 0      # refused before anything changes
    env.set_servo(np.inf, 0.0)
    assert env.level() == 5


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "free"])
@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("pop", POPS)
@pytest.mark.parametrize("rec", RECS)
def test_fp64_emulation_matches_the_patched_oracle(G, emul, rec, pop, envs_per_wave, forced):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8), teacher-forced and
    free-running alike (ten steps of fp64 rounding stay far below them). The limited targets are one subtraction, one compare and one
    add in fp64 on both sides: equal bit for bit."""
    out, (err, flags), serr, lerr = run(emul, G, rec, pop, G["rate"], G["d_gain"], double=True, envs_per_wave=envs_per_wave, forced=forced)
    assert flags == 0
    print(f"{rec} {pop}: max obs/reward error {err.max():.2e}, max state error {serr:.2e}, max limited-target error {lerr:.2e}")
    assert err.max() < 1e-6 and serr < 1e-8, (err.max(), serr)
    assert lerr == 0.0
    # observation slots 48..65 keep this step's own action whatever the servo does to it
    np.testing.assert_array_equal(out[0][0][:, 48:66], G[f"{rec}_{pop}_hist"][1][:, 0])


@pytest.mark.parametrize("pop", POPS)
@pytest.mark.parametrize("rec", RECS)
def test_fp32_emulation_stays_inside_the_fp32_bounds(G, emul, rec, pop):
    """The project's fp32 bounds: median < 5e-6, p99 < 1e-4, teacher-forced."""
    _, (err, flags), _, lerr = run(emul, G, rec, pop, G["rate"], G["d_gain"], double=False)
    assert flags == 0
    print(f"{rec} {pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, limited targets {lerr:.2e}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4
    assert lerr < 1e-6      # a target below 1 rad in float32: half an ulp of the sum and of the rate each, 6e-8 + 6e-8


@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_default_rows_at_level_5_equal_level_0(G, emul, double, envs_per_wave):
    """Latency off: (inf, 0) in every env is no servo model at all, under == in every output."""
    inf, zero = np.full(8, np.inf), np.zeros(8)
    for pop in POPS:
        off, _, _, _ = run(emul, G, "S", pop, None, None, double=double, steps=3, envs_per_wave=envs_per_wave)
        on, _, _, _ = run(emul, G, "S", pop, inf, zero, double=double, steps=3, envs_per_wave=envs_per_wave)
        same(off, on, upto=5)      # (level 0 never touches the limited targets: compare everything else)
        # and level 5 leaves the target of this step's action behind
        a = np.clip(G[f"S_{pop}_actions"][2] * np.float32(0.2), -1, 1).astype(np.float32)
        want = a.astype(np.float64 if double else np.float32) - np.tile([0.0, np.pi / 5, 0.0], 6).astype(np.float64 if double else np.float32)
        np.testing.assert_array_equal(on[2][5], want.astype(np.float64))


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("pop", POPS)
def test_mixed_batch_equals_uniform_batches_bit_for_bit(G, emul, pop, double):
    """Every env is independent: env e of the mixed batch (the fixture's rows under the fixture's delays) equals env e of the batch in which
    EVERY env holds e's row and delay."""
    rate, d_gain, delays, steps = G["rate"], G["d_gain"], G["delays"], 3
    env = emul.EmulServo(1)
    t0 = env.together_count()
    mixed, _, _, _ = run(emul, G, "SL", pop, rate, d_gain, double=double, steps=steps)
    if pop == "stand" and not double:
        assert env.together_count() > t0      # both envs of a wave in ONE constraint pass under different rows
    for e in range(8):
        uni, _, _, _ = run(emul, G, "SL", pop, np.full(8, rate[e]), np.full(8, d_gain[e]), double=double, steps=steps, delays=np.full(8, delays[e], np.int32))
        same(mixed, uni, slice(e, e + 1))


def test_rows_change_the_physics_exactly_where_they_are_set(G, emul):
    def qvel_after(rate, d_gain):
        env = emul.EmulServo(8, double=True, seed=5)
        env.set_servo(rate, d_gain)
        a, cu = load_step(env, G, "S", "drop", 0)
        env.step(a, cmd_u=cu)
        return env.get("qvel")

    diff = np.abs(qvel_after(G["rate"], G["d_gain"]) - qvel_after(None, None)).max(axis=1)
    changed = np.isfinite(G["rate"]) | (G["d_gain"] != 0)
    assert (diff[changed] > 1e-9).all() and (diff[~changed] == 0).all(), diff


def test_physics_only_launch_ignores_the_rows_and_leaves_the_targets_alone(G, emul):
    def after(rate, d_gain):
        env = emul.EmulServo(8, double=False, seed=5)
        env.set_servo(rate, d_gain)
        a, _ = load_step(env, G, "S", "stand", 0)
        l0 = env.servo_state()
        env.step(a, physics_only=True)
        np.testing.assert_array_equal(env.servo_state(), l0)
        return env.get("qpos"), env.get("qvel")

    for u, v in zip(after(G["rate"], G["d_gain"]), after(None, None)):
        np.testing.assert_array_equal(u, v)


def test_standalone_sanitizer_build_of_the_shim_runs_clean(G, emul, tmp_path):
    """The shim as a program of its own (its own main, nothing loaded into Python) under AddressSanitizer and UBSan: one mixed-batch step
    of each population from the SL recording's states, fp32 and fp64; exit status 0 = no report, every value finite, the two-env pass
    taken, no limited target moved faster than its rate."""
    parts = []
    for pop in POPS:
        for k in ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "actions", "hist", "lim"):
            parts.append(np.asarray(G[f"SL_{pop}_{k}"][0], np.float64).ravel())
    states = tmp_path / "states.bin"
    np.concatenate(parts).tofile(states)
    exe = emul.build_program(str(tmp_path / "nm_emul_asan"), (5,), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], opt="-O0")
    r = subprocess.run([exe, "servo", str(states)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "fp32" in r.stdout and "fp64" in r.stdout
