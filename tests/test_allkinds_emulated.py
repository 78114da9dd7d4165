"""All seven kinds of per-env rows on at once - gravity vectors, friction / servo gains, base payloads, actuation latency, the servo
target model, the servo torque limit, the external wrench on the base: what cfg.domain_rand plus cfg.control switches on, level 7 of the
step with every region of the row block non-default - in the host emulation of the device source (tests/emul/nm_emul.cpp), against the
fp64 fixture of the oracle with every kind COMBINED (tests/golden/make_allkinds_goldens.py: per set the library of its payload under
the oracle's rows of the six other kinds). Each kind has such a comparison of its own; this is the one in which the places where the kinds MEET would show: a servo force
formed from a delayed, slew-limited target under the env's own p_gain, with d_gain dof_vel inside the control clip, multiplied by the
env's own kv and only then clamped by the env's torque limit; an implicit factor that leaves out exactly the joints this force saturates
and uses the env's kv; a wrench torque ipos x Rb' F with ipos from the payload's body row under a tilted gravity; and a level-7 launch
reading every region of the row block while wave neighbours differ in every region.

The fp64 emulation of a mixed batch, teacher-forced (every step from the fixture's state, action history AND limited targets) and
free-running; the fp32 emulation inside the fp32 bounds; per ablation (eight: the servo row split into rate and d_gain) the same batch
with that kind at its default values MISSING the fixture in exactly the envs in which the reference itself does; and physics-only
launches, which ignore latency and the servo row but not the limit and the wrench."""
import numpy as np
import pytest

from allkinds_tools import ABLATIONS, POPS, REGIONS, load, nondefault, rows_of, sensitive, set_of


@pytest.fixture(scope="module")
def G():
    return load()


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.WRENCH)
    return em


def make(emul, n, rows, double, envs_per_wave=2, late=True):
    """late False: latency and the servo row off (what a physics-only launch must not read)."""
    env = emul.EmulWrench(n, double=double, seed=5, envs_per_wave=envs_per_wave)
    env.set_env_params(rows["friction"]); env.set_body_params(rows["body"]); env.set_gravity(rows["gravity"])
    env.set_torque_limit(rows["torque"]); env.set_base_wrench(rows["wrench"])
    if late:
        env.set_action_latency(rows["latency"]); env.set_servo(rows["servo"][:, 0], rows["servo"][:, 1])
    assert env.level() == 7 and env.level(True) == 7 and env.layout_agrees()
    return env


def load_step(env, g, pop, t, sets):
    """Start state of step t: env e takes env e % 8 of the trajectory of set sets[e], its action history and limited targets included."""
    ev = np.arange(len(sets)) % 8
    pick = lambda k: g[f"{pop}_{k}"][sets, t, ev]
    env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
    env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
    env.eplen[:] = pick("ep_len")
    env.history[:] = pick("hist")
    env.set_servo_state(pick("lim"))


def run(emul, g, pop, sets, double, envs_per_wave=2, forced=True, without=None):
    """Single steps of one mixed batch. Returns the obs / reward errors [T, n], the state errors [T, n], done flags differing, histories
    differing from the fixture's, the largest limited-target error, two-env constraint passes, env-steps above 16 contacts."""
    n, ev = len(sets), np.arange(len(sets)) % 8
    env = make(emul, n, rows_of(g, sets, without), double, envs_per_wave)
    oerrs, serrs, flags, hist, lerr, ntog, nbig = [], [], 0, 0, 0.0, 0, 0
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
        lerr = max(lerr, float(np.abs(env.servo_state() - g[f"{pop}_lim"][sets, t + 1, ev]).max()))
        ntog += int(env.dbg[0::2, emul.DBG_NTOG].sum())
        nbig += int((env.dbg[:, emul.DBG_NCON] > 16).sum())      # ncon > kMaxCon (16) IS the dispatch to stage_constraint_big (nm_core.h stage_constraint)
    return np.stack(oerrs), np.stack(serrs), flags, hist, lerr, ntog, nbig


def test_the_fixture_mixes_the_kinds(G, emul):
    """What the comparisons below rest on: in a batch of 16 the two envs of a wave differ in every one of the seven regions of the row
    block, the launch takes level 7 with the device's layout agreeing with the host's, the host's batched body rows are the rows of the
    tables the variant oracles were compiled against, and each pooled kind has its default in exactly one set, no set two."""
    sets = set_of(16)
    r = rows_of(G, sets)
    for k in REGIONS:
        a = r[k].reshape(16, -1)
        assert (a[0::2] != a[1::2]).any(axis=1).all(), k
    env = make(emul, 16, r, double=False)
    assert env.level() == 7 and env.layout_agrees()
    np.testing.assert_array_equal(env.torque_rows()[:, :3], r["torque"].astype(np.float32))      # what was set is what the regions hold
    np.testing.assert_array_equal(env.wrench_rows()[:, [0, 1, 2, 4, 5, 6]], r["wrench"].astype(np.float32))
    np.testing.assert_array_equal(np.stack(env.servo(), axis=1), r["servo"].astype(np.float32))
    np.testing.assert_allclose(r["body"], G["body_rows"][sets], rtol=1e-9, atol=1e-15)
    pooled = np.stack([nondefault(G, np.arange(4), kind) for kind in ("gravity", "friction", "payload", "torque", "wrench")])
    assert ((~pooled[:4]).sum(axis=1) == 1).all() and ((~pooled).sum(axis=0) == 1).all() and pooled[4].all()
    for kind, want in zip(ABLATIONS, (12, 12, 12, 12, 12, 10, 12, 16)):
        m = nondefault(G, sets, kind)
        key = {"rate": "servo", "d_gain": "servo"}.get(kind, kind)
        assert m.sum() == want and (rows_of(G, sets, kind)[key][~m] == r[key][~m]).all(), kind
        assert not (sensitive(G, sets, kind, "drop") ^ m).any() and not (sensitive(G, sets, kind, "stand") & ~m).any(), kind
    assert G["grav_rows"][3, 0] != 0 and (G["grav_rows"][3, 4:7] == [0, 0, -9.81]).all()      # set 3 stays unobserved


@pytest.mark.parametrize("envs_per_wave", [2, 1])
@pytest.mark.parametrize("pop", POPS)
def test_fp64_emulation_of_the_combined_batch_matches_the_combined_oracles(G, emul, pop, envs_per_wave):
    """Tolerances: the project's fp64 ones (tests/test_gpu_parity.py: obs / reward < 1e-6, state < 1e-8), no done flag differing, the
    action history equal to the fixture's bit for bit and the limited targets within 1e-12. Teacher-forced and free-running. Two envs per
    wave is the fp32 kernel's layout, one env per wave the fp64 kernel's."""
    sets = set_of(16)
    for forced in (True, False):
        err, serr, flags, hist, lerr, ntog, nbig = run(emul, G, pop, sets, double=True, envs_per_wave=envs_per_wave, forced=forced)
        print(f"{pop} {'forced' if forced else 'free'}: max obs/reward error {err.max():.2e}, max state error {serr.max():.2e}, limited targets {lerr:.2e}, "
              f"two-env passes {ntog}, env-steps above 16 contacts {nbig}")
        assert flags == 0 and hist == 0 and lerr < 1e-12
        assert err.max() < 1e-6 and serr.max() < 1e-8, (err.max(), serr.max())
        if pop == "stand" and envs_per_wave == 2:
            assert ntog > 0
        if pop == "belly":
            assert nbig >= 4


def test_fp32_emulation_is_inside_the_fp32_bounds(G, emul):
    """median < 5e-6 and p99 < 1e-4 (tests/test_gpu_env_params.py), teacher-forced, the four combined sets mixed."""
    sets, errs = set_of(16), []
    for pop in POPS:
        err, _, flags, hist, lerr, _, _ = run(emul, G, pop, sets, double=False)
        print(f"{pop}: fp32 emulation vs fixture: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, limited targets {lerr:.2e}")
        assert flags == 0 and hist == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99))


@pytest.mark.parametrize("kind", ABLATIONS)
def test_a_kind_left_at_its_default_misses_the_fixture(G, emul, kind):
    """The comparison is sensitive to every kind in the emulation too: the fp64 batch with ONE kind at its default values (every kind
    still on, level 7), teacher-forced. In the dropped and in the standing population it leaves the fixture by more than the fp64 state
    tolerance in exactly the envs in which the reference itself does (`sensitive`: the generator's ablation), and every env that carries
    the kind's default stays inside the tolerance."""
    sets = set_of(16)
    dflt = ~nondefault(G, sets, kind)
    for pop in ("drop", "stand"):
        m = sensitive(G, sets, kind, pop)
        _, serr, _, _, _, _, _ = run(emul, G, pop, sets, double=True, without=kind)
        per_env = serr.max(axis=0)
        print(f"{pop} without {kind}: smallest state error of a sensitive env {per_env[m].min():.2e}, largest of any other {per_env[~m].max(initial=0.0):.2e}")
        assert m.any() and not (m & dflt).any()
        assert ((per_env > 1e-8) == m).all() and (per_env[dflt] < 1e-8).all(), per_env


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_physics_only_steps_of_the_combined_batch_ignore_latency_and_the_servo_row(G, emul, double):
    """Physics-only launches at level 7 from the fixture's states with the fixture's delays and servo rows set, its histories and limited
    targets loaded: bit for bit the launches with latency and the servo row off, history and limited targets untouched - and NOT the
    launches with default torque limits or a zero wrench, in the envs the reference marks sensitive."""
    n = 8
    sets = set_of(n)

    def physics(pop, late=True, without=None):
        env = make(emul, n, rows_of(G, sets, without), double, late=late)
        load_step(env, G, pop, 0, sets)
        hist, lim = env.history.copy(), env.servo_state()
        assert hist.any() and lim.any()
        for t in range(3):
            env.step(G[f"{pop}_actions"][sets, t, np.arange(n)], physics_only=True)
        np.testing.assert_array_equal(env.history, hist)
        np.testing.assert_array_equal(env.servo_state(), lim)
        return env.get("qpos"), env.get("qvel"), env.get("qwarm")

    for pop in ("stand", "drop"):
        ref = physics(pop)
        for a, b in zip(ref, physics(pop, late=False)):
            np.testing.assert_array_equal(a, b)
    # (a physics-only launch forms its command from the current joint angles: `drop`, where the limit cuts every env's force)
    for kind in ("torque", "wrench"):
        m, d = sensitive(G, sets, kind, "drop"), ~nondefault(G, sets, kind)
        q = physics("drop", without=kind)[0]
        assert m.any() and (q[m] != ref[0][m]).any(axis=1).all() and (q[d] == ref[0][d]).all(), kind
