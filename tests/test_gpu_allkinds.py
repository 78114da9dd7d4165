"""All seven kinds of per-env rows on at once on the device - gravity vectors, friction / servo gains, base payloads, actuation latency,
the servo target model, the servo torque limit, the external wrench on the base: what cfg.domain_rand plus cfg.control switches on,
level 7 of the step with every region of the row block non-default. Reference: the fp64 fixture of the oracle with every kind COMBINED
(tests/golden/allkinds.npz, make_allkinds_goldens.py: per set the library of its payload under the oracle's rows), which no kernel has a
hand in; uniform batches for what a mixed batch must give (bit for bit: every env is independent). Everything goes through the C ABI's
per-env setters. The fp64 and fp32 emulations of these very states hold the same tolerances on the CPU (tests/test_allkinds_emulated.py)."""
import numpy as np
import pytest
import torch

from allkinds_tools import ABLATIONS, POPS, load, nondefault, rows_of, sensitive, set_of
from test_gpu_env_params import free, load_state, step_errors
from test_gpu_gravity import _run8
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5


@pytest.fixture(scope="module")
def G():
    return load()


def set_rows(env, r):
    """Every kind on, through the per-env setters (the payload as (dm, r): the library derives the body rows)."""
    env.set_gravity(r["gravity"][:, 0:3], r["gravity"][:, 4:7])
    env.set_env_params(mu=r["friction"][:, 0], p_gain=r["friction"][:, 1], kv=r["friction"][:, 2])
    env.set_base_payload(r["payload"][:, 0], r["payload"][:, 1:])
    env.set_action_latency(torch.from_numpy(r["latency"]))
    env.set_servo(r["servo"][:, 0], r["servo"][:, 1])
    env.set_torque_limit(r["torque"])
    env.set_base_wrench(r["wrench"][:, :3], r["wrench"][:, 3:])


def late_state(g, pop, t, sets):
    """(action history, limited targets) at the start of step t."""
    ev = np.arange(len(sets)) % 8
    return g[f"{pop}_hist"][sets, t, ev], g[f"{pop}_lim"][sets, t, ev]


def load_late(env, g, pop, t, sets):
    hist, lim = late_state(g, pop, t, sets)
    env.set_action_history(hist)
    env.set_servo_state(lim)


def differing(env, g, pop, t, sets, tol):
    """(envs whose action history differs from the fixture's at the start of step t, envs whose limited targets lie more than tol away)."""
    hist, lim = late_state(g, pop, t, sets)
    return (int((env.action_history().cpu().numpy() != hist).any(axis=(1, 2)).sum()), int((np.abs(env.servo_state() - lim) > tol).any(axis=1).sum()))


def forced(env, g, pop, sets, steps, tol):
    """test_gpu_env_params.forced with the action history and the limited targets teacher-forced too; returns per-env obs / reward errors
    [steps, n], per-env state errors [steps, n], done flags differing, histories and limited targets differing from the fixture's after
    the step."""
    errs, serrs, flags, hist, lims = [], [], 0, 0, 0
    ev = np.arange(len(sets)) % 8
    for t in range(steps):
        a, cu = load_state(env, g, pop, t, sets)
        load_late(env, g, pop, t, sets)
        env.set_command_uniforms(cu)
        e, _, f = step_errors(env, g, pop, t, sets, env.step(torch.from_numpy(a)))
        q, v, _ = env.get_state()
        serrs.append(np.maximum(np.abs(q - g[f"{pop}_qpos"][sets, t + 1, ev]).max(axis=1), np.abs(v - g[f"{pop}_qvel"][sets, t + 1, ev]).max(axis=1)))
        errs.append(e); flags += f
        h, l = differing(env, g, pop, t + 1, sets, tol)
        hist += h; lims += l
    return np.stack(errs), np.stack(serrs), flags, hist, lims


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the combined oracles
def test_fp64_kernel_with_every_kind_mixed_matches_the_combined_oracles(G):
    """N = 32, the four combined sets mixed over the envs. Teacher-forced single steps and the free-running trajectories of all three
    populations: obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py), no done flag, no history
    row differing, no limited target further than 1e-12 from the fixture's (a subtraction, a compare and an add in fp64 on both sides)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_rows(env, rows_of(G, sets))
    T = G["drop_actions"].shape[1]
    for pop in POPS:
        err, serr, flags, hist, lims = forced(env, G, pop, sets, T, 1e-12)
        print(f"{pop} forced: max obs/reward error {err.max():.2e}, state {serr.max():.2e}")
        assert flags == 0 and hist == 0 and lims == 0 and err.max() < 1e-6 and serr.max() < 1e-8, (pop, err.max(), serr.max(), flags, hist, lims)
        load_late(env, G, pop, 0, sets)
        err, serr, flags = free(env, G, pop, sets, T)
        print(f"{pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, "free", err.max(), serr)
        assert differing(env, G, pop, T, sets, 1e-12) == (0, 0)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. fp32 kernel vs the fixture
def test_fp32_kernel_with_every_kind_mixed_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps, N = 32: median < 5e-6, p99 < 1e-4 (the bounds of tests/test_gpu_env_params.py for the fp32 kernel),
    no done flag differing, no history row differing; the limited targets within 1e-6 (a target below 1 rad in float32: half an ulp of
    the sum and of the rate each, tests/test_servo_emulated.py)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float32, seed=SEED)
    set_rows(env, rows_of(G, sets))
    errs = []
    for pop in POPS:
        err, _, flags, hist, lims = forced(env, G, pop, sets, G[f"{pop}_actions"].shape[1], 1e-6)
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0 and hist == 0 and lims == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    print(f"all populations: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}")
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 3. mixed batch = uniform batches
@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (63, torch.float64), (1, torch.float32), (1, torch.float64)])
def test_mixed_batch_equals_uniform_batches_bit_for_bit_with_every_kind_on(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL carry e's rows of EVERY kind - its gravity, gains, payload,
    delay, servo row, torque limit and wrench (same states, histories, limited targets and actions): what differs between the runs is
    only what e's wave neighbour carries. 8 steps per population, with qacc_warmstart, the action history and servo_state. The uniform
    batches are ALL the (set, e % 8) pairs the batch carries, 16 at N = 63 (every set with four values of e % 8, every value of e % 8 with
    two sets). N = 63: 31 full waves and a half-filled one; the fp32 kernel must have taken both envs of a wave through ONE constraint
    pass, and both kernels an env-step above 16 contacts."""
    sets = set_of(N) if N > 1 else np.array([3])
    rows = rows_of(G, sets)
    ev = np.arange(N) % 8

    def run(env, dbg=None):
        out, ntog, nbig = {}, 0, 0
        for pop in POPS:
            load_late(env, G, pop, 0, sets)
            out[pop], a, b = _run8(env, G, pop, sets, dbg)
            out[pop].append((env.action_history().cpu().numpy(), env.servo_state()))
            ntog += a; nbig += b
        return out, ntog, nbig

    mixed = make_env(N, dtype=dtype, seed=SEED)
    set_rows(mixed, rows)
    dbg = torch.zeros((N, 256), dtype=dtype, device=DEV)
    mixed.set_debug_buffer(dbg)
    runs, ntog, nbig = run(mixed, dbg)
    mixed.set_debug_buffer(None)
    mixed.close()
    print(f"N {N} {dtype}: two-env constraint passes {ntog}, env-steps above 16 contacts {nbig}")
    if N > 1:
        assert nbig >= 1
        if dtype == torch.float32:
            assert ntog >= 1
    carried = sorted({(int(k), int(d)) for k, d in zip(sets, ev)})
    assert N == 1 or (len(carried) == 16 and {k for k, _ in carried} == set(range(4)) and {d for _, d in carried} == set(range(8)))
    for k, d in carried:
        m = (sets == k) & (ev == d)
        e = int(np.flatnonzero(m)[0])
        uni = make_env(N, dtype=dtype, seed=SEED)
        set_rows(uni, {key: np.repeat(v[e:e + 1], N, axis=0) for key, v in rows.items()})
        other, _, _ = run(uni)
        uni.close()
        for pop in POPS:
            for t, (x, y) in enumerate(zip(runs[pop], other[pop])):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart") if len(x) > 2 else ("history", "servo_state"), x, y):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} env {d} {pop} step {t} {name}")


# ------------------------------------------------------------------------------------------------ 4. one ablation per kind
@pytest.mark.parametrize("kind", ABLATIONS)
def test_a_kind_left_at_its_default_misses_the_fixture(G, kind):
    """The comparison of test 1 is sensitive to every kind: the fp64 batch with ONE kind at its default values (the servo row split into
    rate and d_gain), teacher-forced over the standing population. It leaves the fixture by more than the fp64 state tolerance in exactly
    the envs in which the reference itself does (`sensitive`: the generator's ablation), and every env that carries the kind's default
    stays inside the tolerance."""
    sets = set_of(32)
    m, dflt = sensitive(G, sets, kind, "stand"), ~nondefault(G, sets, kind)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_rows(env, rows_of(G, sets, without=kind))
    _, serr, _, _, _ = forced(env, G, "stand", sets, G["stand_actions"].shape[1], 1e-12)
    per_env = serr.max(axis=0)
    print(f"stand without {kind}: smallest state error of a sensitive env {per_env[m].min():.2e}, largest of any other {per_env[~m].max(initial=0.0):.2e}")
    assert m.any() and not (m & dflt).any()
    assert ((per_env > 1e-8) == m).all() and (per_env[dflt] < 1e-8).all(), per_env
    env.close()
