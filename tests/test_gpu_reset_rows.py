"""Per-env rows re-drawn at every reset, from pools (nm_set_reset_rows; nm_reset_rows.h) in every stepping path - reset_idx, step(),
step_tape, policy_play, policy_rollout - BIT FOR BIT: a re-draw copies a pool row into the env's row between two steps, so the per-step
path is compared with a second env object that has no pool and whose rows the test overwrites after every step through the existing
nm_set_* calls, from the numpy restatement of the pick over oracle.rand_u24 (test_reset_rows_host.restated_pick), and every K-step launch
is compared with the per-step path. The only tolerances are the project's for sums that go through float atomics (test_gpu_tape.py).

Episodes have 4 steps (cfg.env.episode_length_s = 0.064) and EPLEN is test_gpu_reset_noise.py's schedule: within 10 steps a wave has both
envs resetting in the same step, only its first, only its second, resets at the last step of a 5-step and of a 10-step launch, and every
env resets twice. Pool sizes (5, 3, 4, 2, 3, 7) in kind order, seed 11; the pool rows are distinct and mild, so a standing robot stays up.
_schedule_is_not_vacuous states, from the restatement alone, that at N = 63 every pool row of every kind is picked at each of k = 0, 1, 2
and that between two consecutive resets 28..55 of the 63 envs change their row in every kind."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_reset_noise import EPLEN, EP_S, K, _actions, _assert_same_state, _assert_same_step, _first_step
from test_gpu_reset_noise import NAMES as NOISE_NAMES, RANGES as NOISE_RANGES
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step
from test_reset_rows_host import ALL_ON, KINDS, WIDTH, restated_pick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
SIZES = (5, 3, 4, 2, 3, 7)


def _pool_values():
    """What set_reset_pool takes per kind: distinct, mild rows - friction 0.6..1.2 and damping 0.7..0.9, payloads <= 0.3 kg, delays
    0..6 substeps, tilts <= 0.1 rad, rates >= 0.2 rad per step, torque limits >= 3 N m."""
    from nightmare_rl_amd.envs.nightmare_v3_env import gravity_from_draw
    return {
        "env_params": dict(mu=np.linspace(0.6, 1.2, 5), kv=np.linspace(0.7, 0.9, 5)),
        "base_payload": dict(dm=np.array([0.1, 0.2, 0.3]), r=np.array([[0.01, 0.0, 0.0], [0.0, -0.015, 0.005], [-0.01, 0.01, 0.01]])),
        "action_latency": dict(substeps=np.array([0, 2, 4, 6], np.int32)),
        "gravity": dict(g=gravity_from_draw(np.zeros((2, 3)), np.array([0.05, 0.1]), np.array([0.5, 2.0]))),
        "servo": dict(rate_limit=np.array([0.2, 0.3, 0.5]), d_gain=np.array([0.0, 0.05, 0.1])),
        "torque_limit": dict(limit=np.array([[3.0 + 0.4 * i, 3.2 + 0.3 * i, 3.0 + 0.2 * i] for i in range(7)])),
    }


def _env(N, dtype=torch.float32, pools=False, offset=0, noise=False, push=False, dr=None):
    """An env with 4-step episodes; pools: all six installed right after construction, before any reset."""
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cfg = NightmareV3Config()
    cfg.env.num_envs, cfg.env.episode_length_s = N, EP_S
    d = dict(dr or {})
    if noise:
        d.update(randomize_reset_state=True, **dict(zip(NOISE_NAMES, NOISE_RANGES)))
    if push:
        d.update(push_robots=True, push_interval_s=0.048, max_push_vel_xy=0.5)          # every 3 steps
    if d:
        cfg.domain_rand = types.SimpleNamespace(**d)
    env = NightmareV3Env(cfg, device=DEV, seed=SEED, env_id_offset=offset, dtype=dtype)
    assert int(env.max_episode_length) == 4
    if pools:
        _install(env)
    return env


def _install(env):
    for kind, values in _pool_values().items():
        env.set_reset_pool(kind, **values)
    assert tuple(env.reset_pool(k)[1] for k in KINDS) == SIZES


def _start(env, offset=0):
    env.reset_idx(None)
    env.episode_length_buf = torch.tensor([EPLEN[(offset + i) % len(EPLEN)] for i in range(env.num_envs)], dtype=torch.int64, device=DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _rows(env):
    """The six kinds' rows as the kernels read them, through the existing getters: [N,3] (mu, p_gain, kv), [N,20], [N] int32, [N,8],
    [N,4], [N,4]."""
    L, h, s, N, real = env._L, env._h, env._stream(), env.num_envs, env._real
    cols = torch.empty(3, N, dtype=real, device=DEV)
    env._ck(L.nm_get_env_params(h, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), s))
    out = [cols.t().contiguous()]
    for kind, get in ((1, L.nm_get_body_params), (2, L.nm_get_action_latency), (3, L.nm_get_gravity), (4, L.nm_get_servo), (5, L.nm_get_torque_limit)):
        t = torch.empty(N, dtype=torch.int32, device=DEV) if kind == 2 else torch.empty(N, WIDTH[kind], dtype=real, device=DEV)
        env._ck(get(h, _ptr(t), s))
        out.append(t)
    return out


def _set_rows(env, rows):
    """Overwrite every env's six rows by hand, through the existing setters of the C ABI (each switches its kind on)."""
    L, h, s = env._L, env._h, env._stream()
    cols = rows[0].t().contiguous()
    env._ck(L.nm_set_env_params(h, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), s))
    for kind, put in ((1, L.nm_set_body_params), (2, L.nm_set_action_latency), (3, L.nm_set_gravity), (4, L.nm_set_servo), (5, L.nm_set_torque_limit)):
        env._ck(put(h, _ptr(rows[kind].contiguous()), s))
    torch.cuda.synchronize()


def _pool_rows(env):
    """The six pools as the device holds them ([P,3] for friction / gains: the pad is not a column of the getter)."""
    p = [env.reset_pool(k)[0] for k in KINDS]
    p[0] = p[0][:, :3].contiguous()
    return p


def _picked(pools, idx):
    """rows of every env from the pools and the test's indices idx [6, N]"""
    return [pools[kind][torch.as_tensor(idx[kind], dtype=torch.int64, device=DEV)] for kind in range(6)]


def _pick_all(envs, k, sizes=SIZES, offset=0):
    """restated indices [6, len(envs)] of reset k[e] of the envs with global ids offset + e"""
    return np.array([restated_pick(SEED, offset + int(e), int(k[e]), sizes) for e in envs], np.int64).T.reshape(6, -1)


def _assert_rows(env, want, what):
    torch.cuda.synchronize()
    for kind, (x, y) in enumerate(zip(_rows(env), want)):
        assert torch.equal(x, y), (what, KINDS[kind])


def _schedule_is_not_vacuous(N=63):
    """From the restatement alone: every pool row of every kind is picked at each of k = 0, 1, 2, and between consecutive resets 28..55
    of the N envs change their row in every kind."""
    idx = [_pick_all(range(N), np.full(N, k)) for k in (0, 1, 2)]
    for k in range(3):
        for kind, P in enumerate(SIZES):
            assert set(idx[k][kind]) == set(range(P)), (k, KINDS[kind])
    for a, b in ((0, 1), (1, 2)):
        for kind in range(6):
            assert 28 <= int((idx[a][kind] != idx[b][kind]).sum()) <= 55, (a, b, KINDS[kind])


def test_the_schedule_is_not_vacuous():
    _schedule_is_not_vacuous()


def _lock_step(ea, eb, N, steps=K):
    """Env A with the six pools, env B without any and the test's overwrites: reset_idx, then `steps` steps of one action stream.
    Returns (the test's reset-row counts, the steps at which each env reset)."""
    pools = _pool_rows(ea)
    k = np.zeros(N, np.int64)
    _start(ea)
    _start(eb)
    idx = _pick_all(range(N), k)
    k += 1
    _set_rows(eb, _picked(pools, idx))
    _assert_rows(ea, _picked(pools, idx), "after reset_idx")
    _assert_same_state(ea, eb, "after reset_idx")
    acts = _actions(steps, N)
    when = [[] for _ in range(N)]
    changed = 0
    for s in range(steps):
        ra, rb = ea.step(acts[s]), eb.step(acts[s])
        ids = np.nonzero(rb[3].cpu().numpy() > 0)[0]
        if len(ids):
            new = _pick_all(ids, k)
            changed += int((new != idx[:, ids]).sum())
            idx[:, ids] = new
            k[ids] += 1
            for e in ids:
                when[e].append(s)
            _set_rows(eb, _picked(pools, idx))
        _assert_same_step(ea, eb, ra, rb, f"step {s}")
        _assert_rows(ea, _picked(pools, idx), f"step {s}")
    assert changed > N                       # the re-draws moved rows
    return k, when


# ------------------------------------------------------------------------------------------------ 1. a re-draw = rows set by hand
@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (1, torch.float32), (63, torch.float64)])
def test_a_redraw_equals_rows_set_by_hand_after_every_step(N, dtype):
    _schedule_is_not_vacuous()
    ea, eb = _env(N, dtype, pools=True), _env(N, dtype)
    k, when = _lock_step(ea, eb, N)
    assert np.array_equal(ea.reset_row_counts(), k) and not eb.reset_row_counts().any()
    assert all(eb.reset_pool(kind) is None for kind in KINDS)
    assert all(len(w) >= 2 for w in when), when
    if N > 1:
        pairs = [(set(when[2 * w]), set(when[2 * w + 1])) for w in range(N // 2)]
        assert any(a & b for a, b in pairs) and any(a - b for a, b in pairs) and any(b - a for a, b in pairs)
        assert 4 in when[6] and 9 in when[6]
    assert not ea.reset_noise_state()[2].any()          # the reset-noise counts are another buffer
    for e in (ea, eb):
        e.close()


def test_lock_step_holds_with_reset_noise_pushes_and_latency_on():
    """Randomised reset states, pushes every 3 steps and a drawn latency on both sides: the re-draw of the rows and the reset draw of the
    state are edits of different words, and a push of step t lands behind both."""
    N = 63
    ea, eb = _env(N, pools=False, noise=True, push=True), _env(N, noise=True, push=True)
    for e in (ea, eb):
        e.draw_action_latency(0, 4)
    _install(ea)
    k, _ = _lock_step(ea, eb, N)
    assert np.array_equal(ea.reset_row_counts(), k) and np.array_equal(ea.reset_noise_state()[2], eb.reset_noise_state()[2])
    assert ea.push_state() == eb.push_state() == (3, 0.5, K)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 2. K-step launches = the per-step path
def _started(N, n, pools=True):
    envs = [_env(N, pools=pools) for _ in range(n)]
    for e in envs:
        _start(e)
        _first_step(e)
    return envs


def _assert_same_rows(ea, eb, what=""):
    torch.cuda.synchronize()
    for kind, (x, y) in enumerate(zip(_rows(ea), _rows(eb))):
        assert torch.equal(x, y), (what, KINDS[kind])
    assert np.array_equal(ea.reset_row_counts(), eb.reset_row_counts()), what


def test_tape_equals_the_per_step_path_and_two_launches_equal_one():
    N = 63
    ea, eb, ec = _started(N, 3)
    (eo,) = _started(N, 1, pools=False)
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb, bc = (_books(N, ep_idx.numel()) for _ in range(3))
    rec, rec2, rec0 = _records(K, N), _records(K, N), _records(K, N)
    k0 = eb.reset_row_counts().astype(np.int64)
    oa = ea.step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(eb, acts, bb, ep_idx)
    for half in (0, 1):
        sl = slice(5 * half, 5 * half + 5)
        oc = ec.step_tape(acts[sl].contiguous(), record={n: rec2[n][sl] for n in rec2}, stats=_stats(bc, ep_idx))
    eo.step_tape(acts, record=rec0)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "done"):
        assert torch.equal(rec[n], per_step[n]), n
        assert torch.equal(rec2[n], per_step[n]), ("two launches", n)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_env(ec, eb, oc, ob)
    _assert_same_books(ba, bb)
    _assert_same_books(bc, bb)
    _assert_same_rows(ea, eb, "tape")
    _assert_same_rows(ec, eb, "two tapes")
    resets = per_step["done"].sum(dim=0).cpu().numpy()
    kb = eb.reset_row_counts().astype(np.int64)
    assert np.array_equal(kb, k0 + resets) and resets.min() >= 2 and k0.min() >= 1
    assert bool(per_step["done"][4].any()) and bool(per_step["done"][K - 1].any())       # resets at a launch's last step
    _assert_rows(ea, _picked(_pool_rows(ea), _pick_all(range(N), kb - 1)), "tape: the rows of the last reset")
    assert not torch.equal(rec["obs"], rec0["obs"])
    for e in (ea, eb, ec, eo):
        e.close()


def test_play_equals_the_per_step_path_and_two_launches_equal_one():
    N = 63
    ac, fu = _networks()
    ea, eb, ec = _started(N, 3)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb, bc = (_books(N, ep_idx.numel()) for _ in range(3))
    oa = ea.policy_play(K, fu.flat, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, False, 77, it, bb, ep_idx)
    for _ in range(2):
        oc = ec.policy_play(5, fu.flat, seed=77, iter_dev=it, stats=_stats(bc, ep_idx))
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_env(ec, eb, oc, ob)
    _assert_same_books(ba, bb)
    _assert_same_books(bc, bb)
    _assert_same_rows(ea, eb, "play")
    _assert_same_rows(ec, eb, "two plays")
    kb = eb.reset_row_counts().astype(np.int64)
    assert kb.min() >= 3
    _assert_rows(ea, _picked(_pool_rows(ea), _pick_all(range(N), kb - 1)), "play: the rows of the last reset")
    for e in (ea, eb, ec):
        e.close()


def test_rollout_equals_the_per_step_path():
    """nm_rollout refuses more steps than an episode has, and an episode has 4 steps here: launches of 4, 4 and 2 steps."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, gamma = 63, 0.99
    ac, fu = _networks()
    ea, eb = _started(N, 2)
    ep_idx = _ep_idx(ea)
    ba, bb = (_books(N, ep_idx.numel()) for _ in range(2))
    o = eb.get_observations()
    for j, T in enumerate((4, 4, 2)):
        it = torch.tensor([3 + j], dtype=torch.int64, device=DEV)
        sa, sb = (_storage(N, T) for _ in range(2))
        oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]))
        for s in range(T):
            act = eb.policy_act(fu.flat, o, 99, it, s, sb)
            o, _, rew, done, infos = eb.step(act)
            _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
        torch.cuda.synchronize()
        for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), (j, name)
        _assert_same_env(ea, eb, oa, o)
        assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
        _assert_same_rows(ea, eb, f"rollout {j}")
    kb = eb.reset_row_counts().astype(np.int64)
    assert kb.min() >= 3
    _assert_rows(ea, _picked(_pool_rows(ea), _pick_all(range(N), kb - 1)), "rollout: the rows of the last reset")
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 3. a one-row pool of the held rows = off
def test_a_one_row_pool_equal_to_the_held_rows_is_the_feature_off():
    """Env Z gets, per kind, a pool of the one row every env holds while the kind is off (the getters' defaults); env O never heard of the
    feature. Per-step and tape, bit for bit; Z counted its resets all the same."""
    N = 63
    ez, eo = _env(N), _env(N)
    dflt = _rows(ez)
    L, h = ez._L, ez._h
    for kind in range(6):
        row = dflt[kind][:1]
        if kind == 0:
            row = torch.cat([row, torch.zeros(1, 1, device=DEV)], dim=1)
        row = row.contiguous()
        ez._ck(L.nm_set_reset_rows(h, kind, _ptr(row), 1, ez._stream()))
        torch.cuda.synchronize()
    for e in (ez, eo):
        _start(e)
    _assert_same_state(ez, eo, "after reset_idx")
    acts = _actions(2 * K, N)
    for s in range(K):
        _assert_same_step(ez, eo, ez.step(acts[s]), eo.step(acts[s]), f"one row, step {s}")
    rz, ro = _records(K, N), _records(K, N)
    oz, oo = ez.step_tape(acts[K:].contiguous(), record=rz), eo.step_tape(acts[K:].contiguous(), record=ro)
    torch.cuda.synchronize()
    for n in rz:
        assert torch.equal(rz[n], ro[n]), n
    _assert_same_env(ez, eo, oz, oo)
    _assert_rows(ez, dflt, "one row")
    assert ez.reset_row_counts().min() >= 5 and not eo.reset_row_counts().any()
    for e in (ez, eo):
        e.close()


# ------------------------------------------------------------------------------------------------ 4. switching on and off, counts
def test_a_pool_installed_later_takes_each_env_at_its_own_reset_and_off_drops_it():
    N = 63
    env = _env(N)
    _start(env)
    acts = _actions(2 * K, N)
    for s in range(3):
        env.step(acts[s])
    dflt = _rows(env)
    _install(env)
    pools = _pool_rows(env)
    _assert_rows(env, dflt, "installing a pool changes no row")
    assert not env.reset_row_counts().any()
    want = [d.clone() for d in dflt]
    k = np.zeros(N, np.int64)
    for s in range(3, 3 + 5):
        done = env.step(acts[s])[3].cpu().numpy() > 0
        ids = np.nonzero(done)[0]
        if len(ids):
            new = _picked(pools, _pick_all(ids, k))
            for kind in range(6):
                want[kind][torch.as_tensor(ids, device=DEV)] = new[kind]
            k[ids] += 1
        _assert_rows(env, want, f"step {s}")
    assert k.min() >= 1 and np.array_equal(env.reset_row_counts(), k)
    # rows set by hand while a pool is installed hold until that env's next reset
    env.set_torque_limit(4.5)
    assert env.reset_pool("torque_limit")[1] == 7 and bool((env.torque_limit() == 4.5).all())
    env.reset_idx([3])
    t = env.torque_limit()
    assert torch.equal(t[3], pools[5][restated_pick(SEED, 3, int(k[3]), SIZES)[5], :3]) and bool((t[4:] == 4.5).all())
    k[3] += 1
    # switching a kind off drops its pool: its rows are the defaults again and stay so through every reset; the others go on
    env.set_torque_limit(None)
    env.set_action_latency(None)
    assert env.reset_pool("torque_limit") is None and env.reset_pool("action_latency") is None
    assert [env.reset_pool(kind)[1] for kind in ("env_params", "base_payload", "gravity", "servo")] == [5, 3, 2, 3]
    env.reset_idx(None)
    idx = _pick_all(range(N), k)
    k += 1
    want = _picked(pools, idx)
    want[2], want[5] = dflt[2], dflt[5]
    _assert_rows(env, want, "after off")
    # dropping a pool alone leaves the rows and the kind as they are
    env.set_reset_pool("servo")
    assert env.reset_pool("servo") is None
    _assert_rows(env, want, "after the drop")
    env.reset_idx(None)
    idx2 = _pick_all(range(N), k)
    k += 1
    want2 = _picked(pools, idx2)
    want2[2], want2[4], want2[5] = dflt[2], want[4], dflt[5]
    _assert_rows(env, want2, "a dropped pool draws no more")
    # counts kept and installed: the next reset of env 5 is draw k[5] + 7
    assert np.array_equal(env.reset_row_counts(), k)
    env.set_reset_row_counts(k + 7)
    assert np.array_equal(env.reset_row_counts(), k + 7)
    env.reset_idx([5])
    i = restated_pick(SEED, 5, int(k[5]) + 7, SIZES)
    rows = _rows(env)
    assert torch.equal(rows[0][5], pools[0][i[0]]) and torch.equal(rows[1][5], pools[1][i[1]]) and torch.equal(rows[3][5], pools[3][i[3]])
    got = env.reset_row_counts()
    assert got[5] == k[5] + 8 and (got[:5] == k[:5] + 7).all()
    with pytest.raises(ValueError, match="num_envs"):
        env.set_reset_row_counts([1, 2, 3])
    env.close()


def test_the_env_refuses_bad_pools_and_changes_nothing():
    from nightmare_rl_amd import _lib
    env = _env(4, pools=True)
    before = _pool_rows(env)
    with pytest.raises(_lib.NightmareHipError, match="nm_set_reset_rows: row 1: mu must be above 1e-5"):
        env.set_reset_pool("env_params", mu=[0.8, 0.0])
    with pytest.raises(_lib.NightmareHipError, match="nm_set_reset_rows: env 2: delay 7"):
        env.set_reset_pool("action_latency", substeps=[0, 1, 7])
    with pytest.raises(_lib.NightmareHipError, match="nm_set_reset_rows: row 0: rate not > 0"):
        env.set_reset_pool("servo", rate_limit=[0.0, 0.3])
    with pytest.raises(_lib.NightmareHipError, match="nm_set_reset_rows: row 2: limit 0 not > 0"):
        env.set_reset_pool("torque_limit", limit=[3.0, 4.0, -1.0, 5.0])
    with pytest.raises(_lib.NightmareHipError, match="nm_set_reset_rows: row 0: a zero gravity_vec"):
        env.set_reset_pool("gravity", g=[0.0, 0.0, -9.81], gravity_vec=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        env.set_reset_pool("base_payload", dm=[-50.0, 0.1])           # model/payload.py refuses the row before the library sees it
    with pytest.raises(ValueError, match="kind must be one of"):
        env.set_reset_pool("terrain", height=[1.0])
    with pytest.raises(ValueError, match="takes mu, p_gain, kv"):
        env.set_reset_pool("env_params", friction=[1.0])
    for x, y in zip(before, _pool_rows(env)):
        assert torch.equal(x, y)
    assert env._L.nm_get_reset_rows(env._h, 0, None, None, env._stream()) == 0            # every out pointer is optional
    env.close()


# ------------------------------------------------------------------------------------------------ 5. sharding
def test_redraws_do_not_depend_on_sharding():
    """One 63-env object against two objects of 32 and 31 envs with env_id_offset 0 and 32: reset_idx, 10 x step(), then a 10-step tape."""
    N, cut = 63, 32
    whole = _env(N, pools=True)
    parts = [_env(cut, pools=True, offset=0), _env(N - cut, pools=True, offset=cut)]
    _start(whole)
    for p, off in zip(parts, (0, cut)):
        _start(p, off)
    sl = [slice(0, cut), slice(cut, N)]

    def same(what):
        torch.cuda.synchronize()
        for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
            np.testing.assert_array_equal(x, np.concatenate(ys), err_msg=what)
        for kind, (x, ys) in enumerate(zip(_rows(whole), zip(*[_rows(p) for p in parts]))):
            assert torch.equal(x, torch.cat(ys)), (what, KINDS[kind])
        assert np.array_equal(whole.reset_row_counts(), np.concatenate([p.reset_row_counts() for p in parts])), what

    same("after reset_idx")
    acts = _actions(2 * K, N)
    for s in range(K):
        rw = whole.step(acts[s])
        rp = [p.step(acts[s, i].contiguous()) for p, i in zip(parts, sl)]
        torch.cuda.synchronize()
        for j in (0, 2, 3):
            assert torch.equal(rw[j], torch.cat([r[j] for r in rp])), (s, j)
        same(f"step {s}")
    rec = _records(K, N)
    whole.step_tape(acts[K:].contiguous(), record=rec)
    recs = [_records(K, p.num_envs) for p in parts]
    for p, i, r in zip(parts, sl, recs):
        p.step_tape(acts[K:, i].contiguous(), record=r)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "done"):
        assert torch.equal(rec[n], torch.cat([r[n] for r in recs], dim=1)), n
    same("after the tape")
    assert whole.reset_row_counts().min() >= 5
    for e in [whole] + parts:
        e.close()


# ------------------------------------------------------------------------------------------------ 6. the config switch, end to end
def test_resample_on_reset_from_the_config_end_to_end():
    """cfg.domain_rand.resample_on_reset with every randomize_* switch on, N = 8, pools of 16 rows: the pools are config_pools' through
    set_reset_pool's conversions, reset() takes every env's first rows from them (k = 0), and 10 steps of 4-step episodes follow the
    restated picks; a second env with another env_id_offset holds the same pools."""
    from nightmare_rl_amd.envs import nightmare_v3_env as ev
    N, P = 8, 16
    dr = dict(resample_on_reset=True, resample_pool_size=P, **ALL_ON)
    env, other = _env(N, dr=dr), _env(N, dr=dr, offset=4096)
    pools = _pool_rows(env)
    assert all(env.reset_pool(kind)[1] == P for kind in KINDS)
    for x, y in zip(pools, _pool_rows(other)):
        assert torch.equal(x, y)
    other.close()
    # the pools are the config's values through the shared helpers
    vals = ev.config_pools(env.cfg, SEED, P, env._envp_default)
    np.testing.assert_array_equal(pools[0][:, 0].cpu().numpy(), vals["env_params"]["mu"].astype(np.float32))
    np.testing.assert_array_equal(pools[2].cpu().numpy(), vals["action_latency"]["substeps"])
    np.testing.assert_array_equal(pools[3][:, 0:3].cpu().numpy(), vals["gravity"]["g"].astype(np.float32))
    np.testing.assert_array_equal(pools[5][:, :3].cpu().numpy(), vals["torque_limit"]["limit"].astype(np.float32))
    rows = ev.payload_body_rows(*ev.payload_values(P, vals["base_payload"]["dm"], vals["base_payload"]["r"], "e"))
    np.testing.assert_array_equal(pools[1].cpu().numpy(), rows.astype(np.float32))
    assert not env.reset_row_counts().any()                     # nothing was drawn once at construction: the rows are the defaults
    sizes = (P,) * 6
    env.reset()
    k = np.ones(N, np.int64)
    idx = _pick_all(range(N), np.zeros(N, np.int64), sizes)
    _assert_rows(env, _picked(pools, idx), "after reset()")
    env.episode_length_buf = torch.tensor(EPLEN, dtype=torch.int64, device=DEV)
    acts = _actions(K, N)
    for s in range(K):
        ids = np.nonzero(env.step(acts[s])[3].cpu().numpy() > 0)[0]
        if len(ids):
            idx[:, ids] = _pick_all(ids, k, sizes)
            k[ids] += 1
        _assert_rows(env, _picked(pools, idx), f"step {s}")
    assert k.min() >= 3 and np.array_equal(env.reset_row_counts(), k)
    env.close()
