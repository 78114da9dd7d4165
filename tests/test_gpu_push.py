"""Push perturbations (nm_set_push; nm_push.h) in the four stepping paths - step(), policy_rollout, policy_play, step_tape - BIT FOR BIT:
a push is an edit of the state between two steps, so the per-step path is compared with a second env object whose qvel[:, 0:2] the test
overwrites through nm_get_state / nm_set_state with a numpy restatement of the draw over oracle.rand_u24, and every K-step launch is
compared with the per-step path. The only tolerances are the project's for sums that go through float atomics (test_gpu_tape.py)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import make_env
from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
PUSH_KEY = 0x50555348          # nm::kPushKey (nm_push.h)


def _draw(seed, N, interval, s, maxv, dtype=np.float32, offset=0):
    """qvel[:, 0:2] of the push at step s (s % interval == 0): u = rand_u24(seed + kPushKey, global env id, 2 (s / interval) + axis),
    v = (2 u - 1) * max in `dtype` (float32: max rounded first; 2 u - 1 is exact, so v is rounded once)."""
    from oracle import oracle as orc
    assert s > 0 and s % interval == 0
    k = s // interval
    u = np.array([[orc.rand_u24((seed + PUSH_KEY) & (2 ** 64 - 1), offset + e, (2 * k + axis) & 0xFFFFFFFF) for axis in (0, 1)] for e in range(N)])
    u = u.astype(dtype)                                           # 24 bits: exact in both
    return (dtype(2) * u - dtype(1)) * dtype(maxv)


def _host_push(env, v):
    qpos, qvel, qw = env.get_state()
    qvel[:, 0:2] = v.astype(np.float64)
    env.set_state(qpos, qvel, qw)


def _actions(K, N, seed=23):
    torch.manual_seed(seed)
    return (torch.rand(K, N, 18) * 2 - 1).to(DEV).contiguous()


def _assert_same_step(ea, eb, ra, rb, what):
    torch.cuda.synchronize()
    assert torch.equal(ra[0], rb[0]), (what, "obs")
    assert torch.equal(ra[2], rb[2]), (what, "reward")
    assert torch.equal(ra[3], rb[3]), (what, "done")
    assert torch.equal(ra[4]["time_outs"], rb[4]["time_outs"]), (what, "time_outs")
    for name, x, y in zip(("qpos", "qvel", "qacc_warmstart"), ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name}")


def _pair(N, dtype=torch.float32, **kw):
    envs = [make_env(N, seed=SEED, dtype=dtype, **kw) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


# ------------------------------------------------------------------------------------------------ 1. a push = a host edit
@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (1, torch.float32), (63, torch.float64)])
def test_push_equals_a_host_edit_of_qvel(N, dtype):
    """Env A: set_push(3, 0.5). Env B: pushes off; before steps 3 and 6 the test overwrites qvel[:, 0:2] with the restated draw. 8 steps of
    one action stream: obs, reward, done, qpos / qvel / qacc_warmstart and extras['time_outs'] agree at every step. fp64: the draw in double."""
    ea, eb = _pair(N, dtype)
    ea.set_push(3, 0.5)
    acts = _actions(8, N)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    pushed = []
    for s in range(8):
        if s in (3, 6):
            v = _draw(SEED, N, 3, s, 0.5, npdt)
            _host_push(eb, v)
            pushed.append(v)
        ra, rb = ea.step(acts[s]), eb.step(acts[s])
        _assert_same_step(ea, eb, ra, rb, f"step {s}")
    assert ea.push_state() == (3, 0.5, 8) and eb.push_state() == (0, 0.0, 9)      # B was never set: it also counted reset()'s step
    assert not np.array_equal(pushed[0], pushed[1]) and np.abs(pushed[0]).max() > 0.05       # the edits were edits
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 2. K-step launches = the per-step path
@pytest.mark.parametrize("N", [63, 130])
def test_tape_with_pushes_equals_the_per_step_path(N):
    """step_tape(K = 8) with interval 3 against 8 x step() with interval 3: the three records row by row, the env afterwards, the books -
    and the run differs from one without pushes (the pushes of steps 3 and 6 happened)."""
    K = 8
    envs = [make_env(N, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
    envs[0].set_push(3, 0.5)
    envs[1].set_push(3, 0.5)
    acts = _actions(K, N)
    ep_idx = _ep_idx(envs[0])
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec = _records(K, N)
    oa = envs[0].step_tape(acts, record=rec, stats=_stats(ba, ep_idx))
    ob, _, per_step = _tape_step_by_step(envs[1], acts, bb, ep_idx)
    rec0 = _records(K, N)
    envs[2].step_tape(acts, record=rec0)
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
    _assert_same_env(envs[0], envs[1], oa, ob)
    _assert_same_books(ba, bb)
    assert envs[0].push_state() == envs[1].push_state() == (3, 0.5, K)
    assert torch.equal(rec["obs"][:3], rec0["obs"][:3])                       # nothing before the first push
    for t in (3, 6):
        assert not torch.equal(rec["obs"][t], rec0["obs"][t]), t
    for e in envs:
        e.close()


@pytest.mark.parametrize("deterministic", [True, False])
def test_play_with_pushes_equals_the_per_step_path(deterministic):
    """policy_play(8) with interval 3 against 8 x [policy_act, step()] with interval 3, as test_gpu_play.py compares them."""
    N, K = 63, 8
    ac, fu = _networks()
    ea, eb = _pair(N)
    for e in (ea, eb):
        e.set_push(3, 0.5)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = ea.policy_play(K, fu.flat, deterministic=deterministic, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, deterministic, 77, it, bb, ep_idx)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    assert ea.push_state() == eb.push_state() == (3, 0.5, K)
    for e in (ea, eb):
        e.close()


def test_rollout_with_pushes_equals_the_per_step_path():
    """policy_rollout(8) into an 8-row storage with interval 3 against 8 x [policy_act, step(), nm_ppo_record] with interval 3: every
    storage row, the env afterwards - and the storage differs from a rollout without pushes from row 4 on (the observation after step 3)."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    N, T, gamma = 63, 8, 0.99
    ac, fu = _networks()
    envs = [make_env(N, seed=SEED) for _ in range(3)]
    for e in envs:
        e.reset()
    envs[0].set_push(3, 0.5)
    envs[1].set_push(3, 0.5)
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(envs[0])
    books = [_books(N, ep_idx.numel()) for _ in envs]
    sts = [_storage(N, T) for _ in envs]
    outs = [envs[k].policy_rollout(T, fu.flat, 99, it, sts[k], gamma, books[k]["cur_ret"], books[k]["cur_len"], books[k]["fin"], ep=(ep_idx, books[k]["ep_acc"]))
            for k in (0, 2)]
    eb, bb, sb = envs[1], books[1], sts[1]
    o = eb.get_observations()
    for s in range(T):
        act = eb.policy_act(fu.flat, o, 99, it, s, sb)
        o, _, rew, done, infos = eb.step(act)
        _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
    torch.cuda.synchronize()
    for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(sts[0], name), getattr(sb, name)), name
    _assert_same_env(envs[0], eb, outs[0], o)
    assert torch.equal(books[0]["cur_ret"], bb["cur_ret"]) and torch.equal(books[0]["cur_len"], bb["cur_len"])
    assert envs[0].push_state() == eb.push_state() == (3, 0.5, T)
    assert torch.equal(sts[0].observations[:4], sts[2].observations[:4]) and not torch.equal(sts[0].observations[4], sts[2].observations[4])
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. the counter runs across launches
def test_push_counter_runs_across_launches_and_starts_where_it_is_told():
    """play(5); play(3) equals play(8). set_push(3, 0.5, start_step=2) pushes the SECOND step of the next launch (index 3): a 4-step tape
    equals step(), host edit with the draw of step 3, 3 x step() on an env without pushes. push_state() = what was set + the steps taken."""
    N = 63
    ac, fu = _networks()
    ea, eb = _pair(N)
    for e in (ea, eb):
        e.set_push(3, 0.5)
    ep_idx = _ep_idx(ea)
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    ea.policy_play(5, fu.flat, seed=5, stats=_stats(ba, ep_idx))
    assert ea.push_state() == (3, 0.5, 5)
    oa = ea.policy_play(3, fu.flat, seed=5, stats=_stats(ba, ep_idx))
    ob = eb.policy_play(8, fu.flat, seed=5, stats=_stats(bb, ep_idx))
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_books(ba, bb)
    assert ea.push_state() == eb.push_state() == (3, 0.5, 8)
    for e in (ea, eb):
        e.close()

    ea, eb = _pair(N)
    ea.set_push(3, 0.5, start_step=2)
    assert ea.push_state() == (3, 0.5, 2)
    acts = _actions(4, N)
    rec = _records(4, N)
    oa = ea.step_tape(acts, record=rec)
    outs = []
    for t in range(4):
        if t == 1:
            _host_push(eb, _draw(SEED, N, 3, 3, 0.5))
        r = eb.step(acts[t])
        outs.append((r[0].clone(), r[2].clone(), r[3].to(torch.uint8)))
    torch.cuda.synchronize()
    for t in range(4):
        assert torch.equal(rec["obs"][t], outs[t][0]) and torch.equal(rec["rew"][t], outs[t][1]) and torch.equal(rec["done"][t], outs[t][2]), t
    _assert_same_env(ea, eb, oa, eb.obs_buf)
    assert ea.push_state() == (3, 0.5, 6)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 4. sharding
def test_pushes_do_not_depend_on_sharding():
    """One 128-env object against two 64-env objects with env_id_offset 0 and 64, interval 3: 7 x step(), then a 7-step tape."""
    whole = make_env(128, seed=SEED)
    parts = [make_env(64, seed=SEED, env_id_offset=off) for off in (0, 64)]
    for e in [whole] + parts:
        e.reset()
        e.set_push(3, 0.5)
    acts = _actions(14, 128)
    for s in range(7):
        rw = whole.step(acts[s])
        rp = [p.step(acts[s, 64 * i:64 * (i + 1)].contiguous()) for i, p in enumerate(parts)]
        torch.cuda.synchronize()
        for k in (0, 2, 3):
            assert torch.equal(rw[k], torch.cat([r[k] for r in rp])), (s, k)
        assert torch.equal(rw[4]["time_outs"], torch.cat([r[4]["time_outs"] for r in rp])), s
        for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
            np.testing.assert_array_equal(x, np.concatenate(ys), err_msg=f"step {s}")
    rec = _records(7, 128)
    whole.step_tape(acts[7:].contiguous(), record=rec)
    recs = [_records(7, 64) for _ in parts]
    for i, p in enumerate(parts):
        p.step_tape(acts[7:, 64 * i:64 * (i + 1)].contiguous(), record=recs[i])
    torch.cuda.synchronize()
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], torch.cat([r[k] for r in recs], dim=1)), k
    for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
        np.testing.assert_array_equal(x, np.concatenate(ys))
    for e in [whole] + parts:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. off is off
def test_off_is_off_and_physics_only_steps_neither_push_nor_count():
    N = 63
    ea, eb = _pair(N)
    ea.set_push(0, 0.5)
    acts = _actions(10, N)
    for s in range(8):
        ra, rb = ea.step(acts[s]), eb.step(acts[s])
        _assert_same_step(ea, eb, ra, rb, f"off, step {s}")
    assert ea.push_state() == (0, 0.5, 8)
    # physics-only launches at a step index that is due (3): no push, no count; the next full step is the one that is pushed
    ea.set_push(3, 0.5, start_step=3)
    for s in (8, 9):
        ea.step_physics(acts[s])
        eb.step_physics(acts[s])
    for x, y in zip(ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y)
    assert ea.push_state() == (3, 0.5, 3)
    _host_push(eb, _draw(SEED, N, 3, 3, 0.5))
    ra, rb = ea.step(acts[0]), eb.step(acts[0])
    _assert_same_step(ea, eb, ra, rb, "the full step after the physics-only ones")
    assert ea.push_state() == (3, 0.5, 4)
    # nm_reset leaves the index alone
    ea.reset_idx(None)
    assert ea.push_state() == (3, 0.5, 4)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 6. the draw is what it says
def test_the_draw_is_uniform_in_range_and_the_kernel_draws_it_at_4096_envs():
    """N = 4096, one push (interval 3, step 3, max 0.5). The library has no push-only entry point, so the values are the restatement's:
    all in [-max, max), the axes differ, per axis |mean| < 5 max / sqrt(3 N) - five standard deviations of the mean of N draws from
    U[-max, max), whose variance is max^2 / 3. The seed is the first one for which the restatement keeps that bound (chosen on the CPU).
    Then the kernel's push with that seed equals the host edit with exactly these values, bit for bit, after the step that follows."""
    N, maxv = 4096, 0.5
    bound = 5 * maxv / math.sqrt(3 * N)
    for seed in range(100, 120):
        v = _draw(seed, N, 3, 3, maxv)
        if (np.abs(v.mean(axis=0, dtype=np.float64)) < bound).all():
            break
    print("seed", seed, "means", v.mean(axis=0, dtype=np.float64), "bound", bound, "min", v.min(), "max", v.max())
    assert v.dtype == np.float32 and v.shape == (N, 2)
    assert (v >= -maxv).all() and (v < maxv).all()
    assert (np.abs(v.mean(axis=0, dtype=np.float64)) < bound).all()
    assert (v[:, 0] != v[:, 1]).mean() > 0.99                  # the two axes draw from different counters
    envs = [make_env(N, seed=seed) for _ in range(2)]
    for e in envs:
        e.reset()
    envs[0].set_push(3, maxv, start_step=3)
    _host_push(envs[1], v)
    a = _actions(1, N)[0]
    ra, rb = envs[0].step(a), envs[1].step(a)
    _assert_same_step(envs[0], envs[1], ra, rb, "4096 envs")
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_push_refuses_what_it_cannot_do():
    from nightmare_rl_amd import _lib
    L = _lib.load()
    env = make_env(4, seed=SEED)
    env.set_push(3, 0.5, start_step=7)
    for args, word in (((-1, 0.5), "interval_steps"), ((3, -0.5), "max_vel_xy"), ((3, float("nan")), "max_vel_xy"), ((3, float("inf")), "max_vel_xy")):
        with pytest.raises(_lib.NightmareHipError, match=word):
            env.set_push(*args)
        assert env.push_state() == (3, 0.5, 7)                   # a refused call changes nothing
    assert L.nm_set_push(None, 3, 0.5, 0) != 0 and b"env" in L.nm_last_error() and b"nm_set_push" in L.nm_last_error()
    assert L.nm_get_push(None, None, None, None) != 0 and b"env" in L.nm_last_error() and b"nm_get_push" in L.nm_last_error()
    assert L.nm_get_push(env._h, None, None, None) == 0          # every out pointer is optional
    env.close()
