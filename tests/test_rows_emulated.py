"""The four kinds of per-env rows together - friction / gains, body rows, actuation latency, gravity vectors - in the host emulation of the
device source (tests/emul/nm_emul.cpp, the one shim), whose layout, default rows, on / off state and level
are the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h): the walk of tests/rows_walk.py over every single-kind transition from
every state of the other three kinds. After every toggle the env that took the walk must be indistinguishable from a fresh env put
directly into that state: the same rows, the same level for full and physics-only launches, and bit-identical steps. N = 3 at two envs
per wave: one full wave and one half-empty one. No tolerance anywhere."""
import numpy as np
import pytest

from conftest import load_golden
from rows_walk import WALK, Walk, check_walk

N, T0 = 3, 2      # envs; the fixture step the start state is taken from (its action history is not zero any more)
ARRAYS = ("qpos", "qvel", "qwarm", "dofpos", "dofvel", "act", "cmd", "epsum", "feetair", "feetflags", "hcache", "rngctr")


@pytest.fixture(scope="module")
def emul():
    from emul import emul as em
    em.build(em.ROWS)
    return em


@pytest.fixture(scope="module")
def G():
    return load_golden("latency.npz")


@pytest.fixture(scope="module")
def SETS():
    """(ENVP_SETS, PAYLOADS, body rows of the payloads, gravity rows): the value sets of the feature suites, from their fixtures."""
    from nightmare_rl_amd.model import payload
    envp, pay = load_golden("env_params.npz")["sets"], load_golden("payload.npz")["sets"]
    return envp, pay, payload.payload_rows(pay[:, 0], pay[:, 1:]), load_golden("gravity.npz")["rows"]


def test_the_walk_is_an_eulerian_circuit_of_the_cube():
    check_walk()


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_device_and_host_agree_on_where_the_latency_words_lie(emul, double):
    """Every accessor of nm_core.h (the device's way) against nm_env_rows.h (the host's), over the whole block: the regions tile it in
    order, with no gap but the pad behind the histories, and the last one ends it."""
    for n in (1, 2, 3, 5, 8, 9):
        assert emul.EmulRows(n, double=double).layout_agrees(), n


def put(env, values, body_of):
    """Switch on exactly the kinds in `values` (a fresh env), or apply them over what is there."""
    if "F" in values:
        env.set_env_params(values["F"])
    if "B" in values:
        env.set_body_params(body_of(values["B"]))
    if "L" in values:
        env.set_action_latency(values["L"])
    if "G" in values:
        env.set_gravity(values["G"])


def load_start(env, g):
    """The dropped population's state of step T0, its action history included, and zero for what the fixture does not carry; returns the
    step's (actions, command uniforms)."""
    pick = lambda k: g[f"drop_{k}"][T0, :N]
    env.set("qpos", pick("qpos")); env.set("qvel", pick("qvel")); env.set("qwarm", pick("qw"))
    env.set("dofpos", pick("dof_pos")); env.set("dofvel", pick("dof_vel")); env.set("act", pick("act")); env.set("cmd", pick("cmd"))
    for k, w in (("epsum", 16), ("feetair", 6), ("feetflags", 1), ("hcache", 8), ("rngctr", 1)):
        env.set(k, np.zeros((N, w)))
    env.eplen[:] = pick("ep_len")
    env.history[:] = pick("hist")
    return pick("actions"), pick("cmd_u").astype(np.float64)


def two_steps(env, g):
    a, cu = load_start(env, g)
    out = list(env.step(a, cmd_u=cu))
    env.step(a, cmd_u=cu, physics_only=True)      # (returns nothing of its own: it shows in the state)
    return out + [env.get(k) for k in ARRAYS] + [env.history.copy(), env.eplen.copy()]


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_an_env_that_took_the_walk_equals_a_fresh_env_put_into_that_state(emul, G, SETS, double):
    envp_sets, payloads, body_rows, grav_rows = SETS
    real = np.float64 if double else np.float32
    body_of = lambda _: body_rows[walk.idx["B"]]      # the body rows of the payloads that are set now
    walker = emul.EmulRows(N, double=double, seed=5)
    f_dflt, b_dflt = envp_sets[0].astype(real), walker.default_body_row()      # (1.0, 20.0, 0.8) are the model's own values: test_env_params_emulated.py
    g_dflt = grav_rows[0].astype(real)      # (0, 0, -9.81) twice: test_gravity_emulated.py
    steps_that_differed = 0
    before = None
    walk = Walk(N, envp_sets, payloads, grav_rows)
    for i, kind, on in walk:
        # the toggle itself: the walker's one kind changes, the others are not touched
        if kind == "F":
            walker.set_env_params(walk.values.get("F"))
        elif kind == "B":
            walker.set_body_params(body_of(walk.values["B"]) if on else None)
        elif kind == "L":
            walker.set_action_latency(walk.values.get("L"))
        else:
            walker.set_gravity(walk.values.get("G"))
        fresh = emul.EmulRows(N, double=double, seed=5)
        put(fresh, walk.values, body_of)
        # (a) the rows: walker = fresh = what was set for the kinds that are on, the defaults / zeros for the kinds that are off
        for physics_only in (False, True):      # L on without G is 2 when physics-only, G on is 4 either way
            assert walker.state(physics_only) == fresh.state(physics_only) == (walk.on(), walk.level(physics_only)), (i, kind, physics_only)
        assert walker.carries_block() == fresh.carries_block() == (walk.level() > 0), (i, kind)
        want = (walk.values["F"].astype(real) if "F" in walk.values else np.tile(f_dflt, (N, 1)),
                body_of(walk.values["B"]).astype(real) if "B" in walk.values else np.tile(b_dflt, (N, 1)),
                walk.values.get("L", np.zeros(N, np.int32)),
                walk.values["G"].astype(real) if "G" in walk.values else np.tile(g_dflt, (N, 1)))
        for w, x, y in zip(want, walker.rows(), fresh.rows()):
            np.testing.assert_array_equal(x, y, err_msg=f"toggle {i} ({kind})")
            np.testing.assert_array_equal(x, w.astype(np.float64) if w.dtype != np.int32 else w, err_msg=f"toggle {i} ({kind})")
        # (b) one step and one physics-only step from the same start: bit-identical
        ow, of = two_steps(walker, G), two_steps(fresh, G)
        for k, (x, y) in enumerate(zip(ow, of)):
            np.testing.assert_array_equal(x, y, err_msg=f"toggle {i} ({kind}), output {k}")
        if before is not None:
            steps_that_differed += any((x != y).any() for x, y in zip(ow, before))
        before = ow
    assert walker.state() == ("", 0) and not walker.carries_block()
    assert (walk.level(True), walk.level()) == (0, 0)
    # the toggles are not no-ops: each changes at least one env's servo gains, base inertia, delay or gravity, which two steps of a moving robot show
    assert steps_that_differed == len(WALK) - 1
