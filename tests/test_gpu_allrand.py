"""All four kinds of per-env rows on at once on the device - gravity vectors, friction / servo gains, base payloads, actuation latency:
what cfg.domain_rand switches on, level 4 of the step with every region of the row block non-default. Reference: the fp64 fixture of the
oracle with every kind COMBINED (tests/golden/allrand.npz, make_allrand_goldens.py: per set the library of its payload under the oracle's rows),
which no kernel has a hand in; uniform batches for what a mixed batch must give (bit for bit: every env is independent). The fp64 and
fp32 emulations of these very states hold the same tolerances on the CPU (tests/test_allrand_emulated.py)."""
import numpy as np
import pytest
import torch

from allrand_tools import KINDS, POPS, load, nondefault, rows_of, set_of
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


def history(g, pop, t, sets):
    return g[f"{pop}_hist"][sets, t, np.arange(len(sets)) % 8]


def forced(env, g, pop, sets, steps):
    """test_gpu_env_params.forced with the action history teacher-forced too; returns per-env obs / reward errors [steps, n], per-env
    state errors [steps, n], done flags differing, histories differing from the fixture's after the step."""
    errs, serrs, flags, hist = [], [], 0, 0
    ev = np.arange(len(sets)) % 8
    for t in range(steps):
        a, cu = load_state(env, g, pop, t, sets)
        env.set_action_history(history(g, pop, t, sets))
        env.set_command_uniforms(cu)
        e, _, f = step_errors(env, g, pop, t, sets, env.step(torch.from_numpy(a)))
        q, v, _ = env.get_state()
        serrs.append(np.maximum(np.abs(q - g[f"{pop}_qpos"][sets, t + 1, ev]).max(axis=1), np.abs(v - g[f"{pop}_qvel"][sets, t + 1, ev]).max(axis=1)))
        errs.append(e); flags += f
        hist += int((env.action_history().cpu().numpy() != history(g, pop, t + 1, sets)).any(axis=(1, 2)).sum())
    return np.stack(errs), np.stack(serrs), flags, hist


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the combined oracles
def test_fp64_kernel_with_every_kind_mixed_matches_the_combined_oracles(G):
    """N = 32, the four combined sets mixed over the envs. Teacher-forced single steps and the free-running trajectories of all three
    populations: obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py), no done flag differing, the
    action history equal to the fixture's."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_rows(env, rows_of(G, sets))
    T = G["drop_actions"].shape[1]
    for pop in POPS:
        err, serr, flags, hist = forced(env, G, pop, sets, T)
        print(f"{pop} forced: max obs/reward error {err.max():.2e}, state {serr.max():.2e}")
        assert flags == 0 and hist == 0 and err.max() < 1e-6 and serr.max() < 1e-8, (pop, err.max(), serr.max())
        env.set_action_history(history(G, pop, 0, sets))
        err, serr, flags = free(env, G, pop, sets, T)
        print(f"{pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, "free", err.max(), serr)
        np.testing.assert_array_equal(env.action_history().cpu().numpy(), history(G, pop, T, sets))
    env.close()


# ------------------------------------------------------------------------------------------------ 2. fp32 kernel vs the fixture
def test_fp32_kernel_with_every_kind_mixed_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps, N = 32: median < 5e-6, p99 < 1e-4 (the bounds of tests/test_gpu_env_params.py for the fp32 kernel),
    no done flag differing."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float32, seed=SEED)
    set_rows(env, rows_of(G, sets))
    errs = []
    for pop in POPS:
        err, _, flags, hist = forced(env, G, pop, sets, G[f"{pop}_actions"].shape[1])
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0 and hist == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 3. mixed batch = uniform batches
@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (63, torch.float64), (1, torch.float32), (1, torch.float64)])
def test_mixed_batch_equals_uniform_batches_bit_for_bit_with_every_kind_on(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL carry e's rows of EVERY kind - its gravity, gains, payload and
    delay (same states, same histories, same actions): what differs between the runs is only what e's wave neighbour carries. 8 steps
    per population. N = 63: 31 full waves and a half-filled one; the fp32 kernel must have taken both envs of a wave through ONE
    constraint pass, and both kernels an env-step above 16 contacts."""
    sets = set_of(N) if N > 1 else np.array([3])
    rows = rows_of(G, sets)

    def run(env, dbg=None):
        out, ntog, nbig = {}, 0, 0
        for pop in POPS:
            env.set_action_history(history(G, pop, 0, sets))
            out[pop], a, b = _run8(env, G, pop, sets, dbg)
            out[pop].append((env.action_history().cpu().numpy(),))
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
    carried = sorted({(int(k), int(d)) for k, d in zip(sets, rows["latency"])})
    assert N == 1 or (len(carried) == 14 and {k for k, _ in carried} == set(range(4)) and {d for _, d in carried} == set(range(7)))      # 14 pairs: every combined set, every delay
    for k, d in carried:
        m = (sets == k) & (rows["latency"] == d)
        e = int(np.flatnonzero(m)[0])
        uni = make_env(N, dtype=dtype, seed=SEED)
        set_rows(uni, {key: np.repeat(v[e:e + 1], N, axis=0) for key, v in rows.items()})
        other, _, _ = run(uni)
        uni.close()
        for pop in POPS:
            for t, (x, y) in enumerate(zip(runs[pop], other[pop])):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart") if len(x) > 1 else ("history",), x, y):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} delay {d} {pop} step {t} {name}")


# ------------------------------------------------------------------------------------------------ 4. one ablation per kind
@pytest.mark.parametrize("kind", KINDS)
def test_a_kind_left_at_its_default_misses_the_fixture(G, kind):
    """The comparison of test 1 is sensitive to every kind: the fp64 batch with ONE kind at its default values, teacher-forced over the
    standing population. Every env that carries a non-default value of that kind leaves the fixture by more than the fp64 state
    tolerance; every env that carries the default stays inside it. (The fp64 emulation: smallest miss 3.6e-2, tests/test_allrand_emulated.py.)"""
    sets = set_of(32)
    m = nondefault(G, sets, kind)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_rows(env, rows_of(G, sets, without=kind))
    _, serr, _, _ = forced(env, G, "stand", sets, G["stand_actions"].shape[1])
    per_env = serr.max(axis=0)
    print(f"stand without {kind}: smallest state error of a non-default env {per_env[m].min():.2e}, largest of a default env {per_env[~m].max():.2e}")
    assert (per_env[m] > 1e-8).all() and (per_env[~m] < 1e-8).all(), per_env
    env.close()
