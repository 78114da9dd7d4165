"""Per-env base payloads (nm_set_body_params / nm_get_body_params / nm_draw_payload) on the device, in every stepping path.
References: the fp64 fixture of the variant oracles (tests/golden/payload.npz, make_payload_goldens.py: the unchanged oracle compiled
against the header of the recompiled model) for what a payload means; uniform batches for what a mixed batch must give (bit for bit:
every env is independent); the per-step path for the K-step launches (bit for bit); a numpy restatement over oracle.rand_u24 for the draw.
The file mirrors tests/test_gpu_env_params.py group for group."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_env_params import DBG_NCON, DBG_NTOG, forced, free, load_state, set_of
from test_gpu_parity import make_env
from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_push import _actions, _assert_same_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 5
POPS = ("drop", "stand", "belly")
PAYLOAD_KEY = 0x5041594C4F     # nm::kPayloadKey (nm_core.h)
ENVP_SETS = np.array([[1.0, 20.0, 0.8], [0.4, 20.0, 0.5], [1.6, 14.0, 0.8], [0.7, 26.0, 1.1]])


@pytest.fixture(scope="module")
def G():
    return load_golden("payload.npz")


def set_payload(env, g, sets):
    s = g["sets"][np.asarray(sets)]
    env.set_base_payload(s[:, 0], s[:, 1:])


# ------------------------------------------------------------------------------------------------ 1. fp64 kernel vs the variant oracles
def test_fp64_kernel_with_mixed_payloads_matches_the_variant_oracles(G):
    """N = 32, the four payload sets mixed over the envs. Teacher-forced single steps and the free-running trajectories of all three
    populations: obs / reward < 1e-6, state < 1e-8 (the project's fp64 tolerances, tests/test_gpu_parity.py), no done flag differing."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float64, seed=SEED)
    set_payload(env, G, sets)
    T = G["drop_actions"].shape[1]
    for pop in POPS:
        err, serr, flags = forced(env, G, pop, sets, T)
        print(f"{pop} forced: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, err.max(), serr)
        err, serr, flags = free(env, G, pop, sets, T)
        print(f"{pop} free {T} steps: max obs/reward error {err.max():.2e}, state {serr:.2e}")
        assert flags == 0 and err.max() < 1e-6 and serr < 1e-8, (pop, "free", err.max(), serr)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. mixed batch = uniform batches
def _run8(env, g, pop, sets, dbg=None):
    """8 free-running steps from the fixture's start states; every step's (obs, rew, done) and state."""
    out = []
    load_state(env, g, pop, 0, sets)
    ev = np.arange(len(sets)) % 8
    ntog = nbig = 0
    for t in range(8):
        env.set_command_uniforms(g[f"{pop}_cmd_u"][sets, t, ev].astype(np.float64))
        r = env.step(torch.from_numpy(g[f"{pop}_actions"][sets, t, ev]))
        out.append((r[0].cpu().numpy().copy(), r[2].cpu().numpy().copy(), r[3].cpu().numpy().copy()) + tuple(env.get_state()))
        if dbg is not None:
            d = dbg.cpu().numpy()
            ntog += int(d[0::2, DBG_NTOG].sum())
            nbig += int((d[:, DBG_NCON] > 16).sum())      # ncon > kMaxCon (16) IS the dispatch to stage_constraint_big (nm_core.h stage_constraint)
    return out, ntog, nbig


@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (63, torch.float64), (1, torch.float32), (1, torch.float64)])
def test_mixed_batch_equals_uniform_batches_bit_for_bit(G, N, dtype):
    """Env e of the mixed batch equals env e of the batch whose envs ALL carry e's payload (same states, same actions): what differs
    between the runs is only what e's wave neighbour carries. 8 steps per population. N = 63: 31 full waves and a half-filled one; the
    fp32 kernel must have taken both envs of a wave through ONE constraint pass, and both kernels an env-step above 16 contacts."""
    sets = set_of(N) if N > 1 else np.array([3])
    mixed = make_env(N, dtype=dtype, seed=SEED)
    set_payload(mixed, G, sets)
    dbg = torch.zeros((N, 256), dtype=dtype, device=DEV)
    mixed.set_debug_buffer(dbg)
    runs, ntog, nbig = {}, 0, 0
    for pop in POPS:
        runs[pop], a, b = _run8(mixed, G, pop, sets, dbg)
        ntog += a; nbig += b
    mixed.set_debug_buffer(None)
    mixed.close()
    print(f"N {N} {dtype}: two-env constraint passes {ntog}, env-steps above 16 contacts {nbig}")
    if N > 1:
        assert nbig >= 1
        if dtype == torch.float32:
            assert ntog >= 1
    for k in sorted(set(sets.tolist())):
        uni = make_env(N, dtype=dtype, seed=SEED)
        set_payload(uni, G, np.full(N, k))
        m = sets == k
        for pop in POPS:
            other, _, _ = _run8(uni, G, pop, sets)
            for t, (x, y) in enumerate(zip(runs[pop], other)):
                for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart"), x, y):
                    np.testing.assert_array_equal(u[m], v[m], err_msg=f"set {k} {pop} step {t} {name}")
        uni.close()


# ------------------------------------------------------------------------------------------------ 3. fp32 kernel vs the fixture
def test_fp32_kernel_with_mixed_payloads_is_within_the_fp32_bounds(G):
    """Teacher-forced single steps, N = 32: median < 5e-6, p99 < 1e-4 (the bounds of tests/test_gpu_env_params.py for the fp32 kernel; the
    fp32 emulation of these very states stays inside them, tests/test_payload_emulated.py)."""
    sets = set_of(32)
    env = make_env(32, dtype=torch.float32, seed=SEED)
    set_payload(env, G, sets)
    errs = []
    for pop in POPS:
        err, _, flags = forced(env, G, pop, sets, G[f"{pop}_actions"].shape[1])
        print(f"{pop}: median {np.median(err):.2e}, p99 {np.percentile(err, 99):.2e}, max {err.max():.2e}, done flags differing {flags}")
        assert flags == 0
        errs.append(err.ravel())
    err = np.concatenate(errs)
    assert np.median(err) < 5e-6 and np.percentile(err, 99) < 1e-4, (np.median(err), np.percentile(err, 99), err.max())
    env.close()


# ------------------------------------------------------------------------------------------------ 4. off = never set
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_never_set_default_rows_and_set_then_cleared_are_bit_identical(dtype):
    from nightmare_rl_amd import _lib
    import ctypes as C
    N = 63
    envs = [make_env(N, dtype=dtype, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
    rows = envs[1].base_payload()["rows"]                       # nm_get_body_params while off: the model's own row for every env
    assert rows.dtype == dtype and rows.shape == (N, 20) and bool((rows == rows[0]).all())
    envs[1]._ck(envs[1]._L.nm_set_body_params(envs[1]._h, C.c_void_p(rows.data_ptr()), envs[1]._stream()))     # ... set explicitly: level 2
    envs[2].set_base_payload(0.5, [0.03, 0.0, 0.04])
    assert not torch.equal(envs[2].base_payload()["rows"], rows)
    envs[2].set_base_payload()                                  # off again
    for e in envs:
        assert torch.equal(e.base_payload()["rows"], rows)
    # rows the library refuses, before anything of the env changes
    for col, word in ((9, "mass"), (10, "total_mass"), (3, "inertia"), (12, "invweight0"), (18, "pgs_scale")):
        bad = rows.clone()
        bad[5, col] = -1.0 if col != 10 else 0.5 * float(rows[5, 9])
        with pytest.raises(_lib.NightmareHipError, match=word):
            envs[0]._ck(envs[0]._L.nm_set_body_params(envs[0]._h, C.c_void_p(bad.data_ptr()), envs[0]._stream()))
    acts = _actions(8, N)
    for s in range(8):
        r = [e.step(acts[s]) for e in envs]
        _assert_same_step(envs[0], envs[1], r[0], r[1], f"default rows, step {s}")
        _assert_same_step(envs[0], envs[2], r[0], r[2], f"set then cleared, step {s}")
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. every stepping path
def _mixed_pair(G, N, n=2):
    envs = [make_env(N, seed=SEED) for _ in range(n)]
    for e in envs:
        e.reset()
        set_payload(e, G, set_of(N))
    return envs


@pytest.mark.parametrize("N", [63, 130])
def test_tape_with_payloads_equals_the_per_step_path(G, N):
    K = 8
    ea, eb, e0 = _mixed_pair(G, N, 3)
    e0.set_base_payload()
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec, rec0 = _records(K, N), _records(K, N)
    oa = ea.step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(eb, acts, bb, ep_idx)
    e0.step_tape(acts, record=rec0)
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    assert not torch.equal(rec["obs"][-1], rec0["obs"][-1])               # the payloads were honoured
    assert torch.equal(rec["obs"][-1][0::16], rec0["obs"][-1][0::16])     # ... and env 0, 16, ... carry none: untouched
    for e in (ea, eb, e0):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
@pytest.mark.parametrize("deterministic", [True, False])
def test_play_with_payloads_equals_the_per_step_path(G, N, deterministic):
    K = 8
    ac, fu = _networks()
    ea, eb = _mixed_pair(G, N)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
def test_rollout_with_payloads_equals_the_per_step_path(G, N):
    from nightmare_rl_amd import _lib
    L = _lib.load()
    T, gamma = 8, 0.99
    ac, fu = _networks()
    ea, eb = _mixed_pair(G, N)
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    sa, sb = _storage(N, T), _storage(N, T)
    oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]))
    o = eb.get_observations()
    for s in range(T):
        act = eb.policy_act(fu.flat, o, 99, it, s, sb)
        o, _, rew, done, infos = eb.step(act)
        _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
    torch.cuda.synchronize()
    for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(sa, name), getattr(sb, name)), name
    _assert_same_env(ea, eb, oa, o)
    assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 6. with friction and gains
def test_payload_with_friction_and_gains_equals_the_uniform_runs(G):
    """Both kinds of rows set, mixed independently over the envs: env e equals the run in which every env carries e's payload AND e's
    friction / gains. And the payload alone (the host then supplies default friction / gain rows) equals the same payload with those
    rows set explicitly at their defaults. fp32, bit for bit, 8 steps of the standing population."""
    N = 16
    sets, esets = set_of(N), (set_of(N) + 1 + np.arange(N) // 8) % 4
    combos = sorted({(int(a), int(b)) for a, b in zip(sets, esets)})
    assert len(combos) >= 6

    def run(psets, rows):
        env = make_env(N, seed=SEED)
        set_payload(env, G, psets)
        if rows is not None:
            env.set_env_params(mu=rows[:, 0], p_gain=rows[:, 1], kv=rows[:, 2])
        out, _, _ = _run8(env, G, "stand", sets)
        env.close()
        return out

    mixed = run(sets, ENVP_SETS[esets])
    for a, b in combos:
        uni = run(np.full(N, a), np.repeat(ENVP_SETS[b][None], N, axis=0))
        m = (sets == a) & (esets == b)
        for t, (x, y) in enumerate(zip(mixed, uni)):
            for name, u, v in zip(("obs", "rew", "done", "qpos", "qvel", "qacc_warmstart"), x, y):
                np.testing.assert_array_equal(u[m], v[m], err_msg=f"payload {a} params {b} step {t} {name}")
    alone, both = run(sets, None), run(sets, np.repeat(ENVP_SETS[0][None], N, axis=0))
    for x, y in zip(alone, both):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------------------------------------ 7. the draw
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_draw_is_its_numpy_restatement_and_lies_in_range(dtype):
    from oracle import oracle as orc
    from nightmare_rl_amd import _lib
    N, npdt = 1024, (np.float64 if dtype == torch.float64 else np.float32)
    env = make_env(N, dtype=dtype, seed=SEED, env_id_offset=1000)
    ma, co = (-0.2, 1.0), (-0.01, 0.01)      # (a negative mass far from the base's COM is not an admissible body: model/payload.py refuses it)
    p = env.draw_base_payload(mass_range=ma, com_range=co)
    got = np.concatenate([p["dm"][:, None], p["r"]], axis=1)
    lo = np.array([ma[0], co[0], co[0], co[0]]).astype(npdt)
    hi = np.array([ma[1], co[1], co[1], co[1]]).astype(npdt)
    for c in range(4):
        u = np.array([orc.rand_u24((SEED + PAYLOAD_KEY) & (2 ** 64 - 1), 1000 + e, c) for e in range(N)]).astype(npdt)      # 24 bits: exact
        want = lo[c] + u * (hi[c] - lo[c])                       # numpy rounds the product, then the sum: what the kernel is written to do
        assert want.dtype == npdt
        np.testing.assert_array_equal(got[:, c], want.astype(np.float64), err_msg=f"column {c}")
        assert got[:, c].min() >= lo[c] and got[:, c].max() <= hi[c] and got[:, c].max() - got[:, c].min() > 0.98 * (float(hi[c]) - float(lo[c]))
    # the rows that were set are the host derivation of the draw
    from nightmare_rl_amd.model import payload
    want_rows = torch.from_numpy(payload.payload_rows(got[:, 0], got[:, 1:])).to(dtype)
    assert torch.equal(p["rows"].cpu(), want_rows)
    # refusals before any device call; a refused call changes nothing
    for kw in (dict(mass_range=(0.5, 0.1)), dict(mass_range=(0.0, float("inf"))), dict(com_range=(float("nan"), 0.1))):
        with pytest.raises(_lib.NightmareHipError, match="nm_draw_payload"):
            env.draw_base_payload(**kw)
    with pytest.raises(ValueError, match="mass must stay positive"):
        env.set_base_payload(-2.0)
    assert torch.equal(env.base_payload()["rows"], p["rows"])
    env.close()


def test_drawn_payloads_and_results_do_not_depend_on_sharding():
    whole = make_env(128, seed=SEED)
    parts = [make_env(64, seed=SEED, env_id_offset=off) for off in (0, 64)]
    for e in [whole] + parts:
        e.reset()
        e.draw_base_payload(mass_range=(-0.2, 1.0), com_range=(-0.01, 0.01))
    pw, pp = whole.base_payload(), [p.base_payload() for p in parts]
    assert torch.equal(pw["rows"], torch.cat([p["rows"] for p in pp]))
    np.testing.assert_array_equal(pw["dm"], np.concatenate([p["dm"] for p in pp]))
    assert np.unique(pw["dm"]).size > 100
    acts = _actions(8, 128)
    for s in range(8):
        rw = whole.step(acts[s])
        rp = [p.step(acts[s, 64 * i:64 * (i + 1)].contiguous()) for i, p in enumerate(parts)]
        torch.cuda.synchronize()
        for k in (0, 2, 3):
            assert torch.equal(rw[k], torch.cat([r[k] for r in rp])), (s, k)
        for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
            np.testing.assert_array_equal(x, np.concatenate(ys), err_msg=f"step {s}")
    for e in [whole] + parts:
        e.close()


def test_cfg_domain_rand_draws_at_construction():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env

    class Cfg(NightmareV3Config):
        class domain_rand:
            randomize_base_mass, added_mass_range = True, [-0.2, 1.0]
            randomize_com_displacement, com_displacement_range = True, [-0.01, 0.01]

    cfg = Cfg()
    cfg.env.num_envs = 256
    env = NightmareV3Env(cfg, device=DEV, seed=SEED)
    p = env.base_payload()
    assert -0.2 <= p["dm"].min() and p["dm"].max() <= 1.0 and p["dm"].max() - p["dm"].min() > 0.6          # half the range
    assert -0.01 <= p["r"].min() and p["r"].max() <= 0.01 and (p["r"].max(axis=0) - p["r"].min(axis=0) > 0.01).all()
    first = p["rows"].clone()
    assert first.unique(dim=0).shape[0] == 256
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(256, 18, device=DEV))
    assert torch.equal(env.base_payload()["rows"], first)              # drawn once: resets and steps leave them alone
    env.close()


# ------------------------------------------------------------------------------------------------ 8. physical sanity
def test_a_heavier_base_settles_lower(G):
    """Zero actions from the reset pose until the robot has settled (150 steps): the contacts are soft (solref 0.02), so the base of an env
    carrying +1.0 kg comes to rest below that of an env carrying -0.3 kg. An ordering only. (The fp32 emulation of this very run: base
    origin at 0.09235 m against 0.09384 m; the fp64 oracle's settled states of the fixture: the same to 1e-7 m.)"""
    N = 8
    sets = np.array([3, 2] * 4)
    np.testing.assert_array_equal(G["sets"][[3, 2], 0], [1.0, -0.3])
    env = make_env(N, seed=SEED)
    env.reset()
    set_payload(env, G, sets)
    a = torch.zeros((N, 18))
    for _ in range(150):
        env.step(a)
    q, v, _ = env.get_state()
    heavy, light = q[sets == 3, 2].mean(), q[sets == 2, 2].mean()
    print("settled base height: +1.0 kg ->", heavy, " -0.3 kg ->", light)
    print("largest velocity left:", np.abs(v).max())
    assert env.counters()["bad_state_resets"] == 0
    assert heavy < light
    env.close()
