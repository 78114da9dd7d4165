"""All four kinds of per-env rows on at once - gravity vectors, friction / servo gains, base payloads, actuation latency: what
cfg.domain_rand switches on, level 4 of the step with every region of the row block non-default - in the host emulation of the device
source (tests/emul/nm_emul.cpp), against the fp64 fixture of the oracle with every kind COMBINED (tests/golden/make_allrand_goldens.py: per
set the library of its payload under the oracle's rows of every other kind). Each kind has such a comparison of its own; this is the one in which a step that
read a neighbouring region's words, applied the late command with the default gain or built the base block from the default inertial
position would show: the kinds meet in the subtree centre of mass (body mass and total mass under the env's gravity), the base bias, the
servo stage (the env's gain on a delayed action) and the epilogue (the env's own gravity_vec).

The fp64 emulation of a mixed batch, teacher-forced (every step from the fixture's state AND action history) and free-running; the fp32
emulation inside the fp32 bounds; per kind, the same batch with that kind at its default values MISSING the fixture; and physics-only
launches, which ignore latency."""
import numpy as np
import pytest

from allrand_tools import KINDS, POPS, load, nondefault, rows_of, set_of


@pytest.fixture(scope="module")
def G():
    return load()


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.ROWS)
    return em


def make(emul, n, rows, double, envs_per_wave=2, latency=True):
    env = emul.EmulRows(n, double=double, seed=5, envs_per_wave=envs_per_wave)
    env.set_env_params(rows["friction"]); env.set_body_params(rows["body"]); env.set_gravity(rows["gravity"])
    if latency:
        env.set_action_latency(rows["latency"])
    assert env.state() == ("FBLG" if latency else "FBG", 4)
    return env


def load_step(env, g, pop, t, sets):
    """Start state of step t: env e takes env e % 8 of the trajectory of set sets[e], its action history included."""
    ev = np.arange(len(sets)) % 8
    pick = lambda k: g[f"{pop}_{k}"][sets, t, ev]
    env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
    env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
    env.eplen[:] = pick("ep_len")
    env.history[:] = pick("hist")


def run(emul, g, pop, sets, double, envs_per_wave=2, forced=True, without=None):
    """Single steps of one mixed batch. Returns the obs / reward errors [T, n], the state errors [T, n], done flags differing, histories
    differing from the fixture's, two-env constraint passes, env-steps above 16 contacts."""
    n, ev = len(sets), np.arange(len(sets)) % 8
    env = make(emul, n, rows_of(g, sets, without), double, envs_per_wave)
    oerrs, serrs, flags, hist, ntog, nbig = [], [], 0, 0, 0, 0
    for t in range(g[f"{pop}_actions"].shape[1]):
        if forced or t == 0:
            load_step(env, g, pop, t, sets)
        obs, rew, done, _ = env.step(g[f"{pop}_actions"][sets, t, ev], cmd_u=g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64), want_dbg=True)
        oe = np.abs(obs.astype(np.float64) - g[f"{pop}_obs"][sets, t, ev]).max(axis=1)
        re_ = np.abs(rew.astype(np.float64) - g[f"{pop}_rew"][sets, t, ev])
        oerrs.append(np.maximum(oe, re_))
        serrs.append(np.maximum(np.abs(env.get("qpos") - g[f"{pop}_qpos"][sets, t + 1, ev]).max(axis=1), np.abs(env.get("qvel") - g[f"{pop}_qvel"][sets, t + 1, ev]).max(axis=1)))
        flags += int((done != g[f"{pop}_done"][sets, t, ev]).sum())
        hist += int((env.history != g[f"{pop}_hist"][sets, t + 1, ev]).any(axis=(1, 2)).sum())
        ntog += int(env.dbg[0::2, emul.DBG_NTOG].sum())
        nbig += int((env.dbg[:, emul.DBG_NCON] > 16).sum())      # ncon > kMaxCon (16) IS the dispatch to stage_constraint_big (nm_core.h stage_constraint)
    return np.stack(oerrs), np.stack(serrs), flags, hist, ntog, nbig


def test_the_fixture_mixes_the_kinds(G):
    """What the comparisons below rest on: in a batch of 16 no two kinds are aligned, neighbours in a wave differ in every kind, and the
    host's batched body rows are the rows of the tables the variant oracles were compiled against."""
    sets = set_of(16)
    np.testing.assert_array_equal(G["sets"], [[k, (k + 1) % 4, (k + 2) % 4] for k in range(4)])
    r = rows_of(G, sets)
    for k in ("gravity", "friction", "body", "latency"):
        a = r[k].reshape(16, -1)
        assert (a[0::2] != a[1::2]).any(axis=1).all(), k
    np.testing.assert_allclose(r["body"], G["body_rows"][sets], rtol=1e-9, atol=1e-15)
    for kind in KINDS:
        m = nondefault(G, sets, kind)
        assert m.sum() == 12 and (rows_of(G, sets, kind)[kind][~m] == r[kind][~m]).all()
    assert G["grav_rows"][3, 0] != 0 and (G["grav_rows"][3, 4:7] == [0, 0, -9.81]).all()      # set 3 stays unobserved


@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("pop", POPS)
def test_fp64_emulation_of_the_combined_batch_matches_the_combined_oracles(G, emul, pop, envs_per_wave):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8), no done flag differing, the
    action history equal to the fixture's. Teacher-forced and free-running. Two envs per wave is the fp32 kernel's layout, one env per
    wave the fp64 kernel's."""
    sets = set_of(16)
    for forced in (True, False):
        err, serr, flags, hist, ntog, nbig = run(emul, G, pop, sets, double=True, envs_per_wave=envs_per_wave, forced=forced)
        print(f"{pop} {'forced' if forced else 'free'}: max obs/reward error {err.max():.2e}, max state error {serr.max():.2e}, two-env passes {ntog}, env-steps above 16 contacts {nbig}")
        assert flags == 0 and hist == 0
        assert err.max() < 1e-6 and serr.max() < 1e-8, (err.max(), serr.max())
        if pop == "stand" and envs_per_wave == 2:
            assert ntog > 0
        if pop == "belly":
            assert nbig >= 4


def test_fp32_emulation_is_inside_the_fp32_bounds(G, emul):
    """median < 5e-6 and p99 < 1e-4 (tests/test_gpu_env_params.py), teacher-forced, the four combined sets mixed."""
    sets, errs = set_of(16), []
    for pop in POPS:
        err, _, flags, hist, _, _ = run(emul, G, pop, sets, double=False)
        print(f"{pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}")
        assert flags == 0 and hist == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99))


@pytest.mark.parametrize("kind", KINDS)
def test_a_kind_left_at_its_default_misses_the_fixture(G, emul, kind):
    """The comparison is sensitive to every kind in the emulation too: the fp64 batch with ONE kind at its default values (the kind still
    on, level 4), teacher-forced. Every env that carries a non-default value of that kind leaves the fixture by more than the fp64 state
    tolerance in the dropped and in the standing population; every env that carries the default stays inside it."""
    sets = set_of(16)
    m = nondefault(G, sets, kind)
    for pop in ("drop", "stand"):
        _, serr, _, _, _, _ = run(emul, G, pop, sets, double=True, without=kind)
        per_env = serr.max(axis=0)
        print(f"{pop} without {kind}: smallest state error of a non-default env {per_env[m].min():.2e}, largest of a default env {per_env[~m].max():.2e}")
        assert (per_env[m] > 1e-8).all() and (per_env[~m] < 1e-8).all(), per_env


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_physics_only_steps_of_the_combined_batch_ignore_latency(G, emul, double):
    """Physics-only launches at level 4 from the fixture's states with the fixture's delays set and its histories loaded: bit for bit the
    launches with latency off, the history untouched - and NOT the launches with default gravity, gains or payload."""
    n = 8
    sets = set_of(n)

    def physics(latency=True, without=None):
        env = make(emul, n, rows_of(G, sets, without), double, latency=latency)
        load_step(env, G, "stand", 0, sets)
        hist = env.history.copy()
        assert hist.any()
        for t in range(3):
            env.step(G["stand_actions"][sets, t, np.arange(n)], physics_only=True)
        np.testing.assert_array_equal(env.history, hist)
        return env.get("qpos"), env.get("qvel"), env.get("qwarm")

    ref = physics()
    for a, b in zip(ref, physics(latency=False)):
        np.testing.assert_array_equal(a, b)
    for kind in KINDS[:3]:
        m = nondefault(G, sets, kind)
        q = physics(without=kind)[0]
        assert (q[m] != ref[0][m]).any(axis=1).all() and (q[~m] == ref[0][~m]).all(), kind
