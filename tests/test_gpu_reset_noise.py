"""Randomised reset states (nm_set_reset_noise; nm_reset_noise.h) in every stepping path - reset_idx, step(), step_tape, policy_play,
policy_rollout - BIT FOR BIT: a reset draw is an edit of the state between two steps, so the per-step path is compared with a second env
object whose rows the test overwrites through get_state / set_state with the numpy restatement of the draw over oracle.rand_u24
(test_reset_noise_host.restated_offsets), and every K-step launch is compared with the per-step path. The only tolerances are the
project's for sums that go through float atomics (test_gpu_tape.py).

Every env is built with cfg.env.episode_length_s = 0.064: 4 steps at dt = 0.016 (the constructor admits the product: 0.064 / 0.016 = 4.0
in doubles), so an env whose episode_length_buf holds e times out at steps 4 - e and 9 - e of a 10-step run. EPLEN assigns e per env so
that within 10 steps wave 0 has both envs resetting in the same step, wave 1 only its first env (step 1) and only its second (step 3),
wave 2 the other way round, envs 6 and 14, ... reset at steps 4 and 9 (the last step of a 5-step and of a 10-step launch), and every
env resets twice. The K-step tests take reset()'s zero-action step first (_first_step), which shifts that schedule by one step: there the
envs with e = 4 reset in that step and again at steps 4 and 9 of the launch - its last step, and the last step of a 5-step launch."""
import types

import numpy as np
import pytest
import torch

from test_gpu_play import _assert_same_books, _books, _ep_idx, _networks, _stats, _storage
from test_gpu_play import _step_by_step as _play_step_by_step
from test_gpu_rollout import _record
from test_gpu_tape import _assert_same_env, _records
from test_gpu_tape import _step_by_step as _tape_step_by_step
from test_reset_noise_host import restated_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
EP_S = 0.064
K = 10
EPLEN = (4, 4, 3, 1, 1, 3, 0, 2)
# base_height only upwards (the feet stay off the floor at the start), the rest symmetric and small enough for a standing robot
RANGES = ((0.0, 0.03), (-0.15, 0.15), (-0.3, 0.3), (-0.3, 0.3), (-0.8, 0.8))
NAMES = ("reset_base_height_range", "reset_dof_pos_range", "reset_base_lin_vel_range", "reset_base_ang_vel_range", "reset_dof_vel_range")


def _env(N, dtype=torch.float32, ranges=None, offset=0, push=False):
    """An env with 4-step episodes; ranges: the feature on from construction, through the optional cfg.domain_rand."""
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    cfg = NightmareV3Config()
    cfg.env.num_envs, cfg.env.episode_length_s = N, EP_S
    dr = {}
    if ranges is not None:
        dr.update(randomize_reset_state=True, **dict(zip(NAMES, ranges)))
    if push:
        dr.update(push_robots=True, push_interval_s=0.048, max_push_vel_xy=0.5)          # every 3 steps
    if dr:
        cfg.domain_rand = types.SimpleNamespace(**dr)
    env = NightmareV3Env(cfg, device=DEV, seed=SEED, env_id_offset=offset, dtype=dtype)
    assert int(env.max_episode_length) == 4
    return env


def _start(env, offset=0):
    """reset_idx(all) - draw 0 of every env while the feature is on - and the episode lengths of the module's docstring."""
    env.reset_idx(None)
    N = env.num_envs
    env.episode_length_buf = torch.tensor([EPLEN[(offset + i) % len(EPLEN)] for i in range(N)], dtype=torch.int64, device=DEV)


def _first_step(env):
    """the zero-action step of reset(): the K-step launches start from its observation"""
    return env.step(torch.zeros(env.num_envs, 18, device=DEV))


def _actions(Kk, N, seed=23):
    torch.manual_seed(seed)
    return (torch.rand(Kk, N, 18) * 2 - 1).to(DEV).contiguous()


def _host_edit(env, ids, k, npdt, offset=0):
    """The rows of envs `ids`, which a reset has just set to qpos0 / zero velocity, overwritten as the feature defines it, with the draw
    of reset k[e]; k is advanced. Returns the offsets used, [len(ids), 43]."""
    qpos, qvel, qw = env.get_state()
    used = []
    for e in ids:
        d = restated_offsets(RANGES, SEED, offset + int(e), int(k[e]), npdt)
        qpos[e, 2] = npdt(qpos[e, 2]) + d[0]
        qpos[e, 7:25] = qpos[e, 7:25].astype(npdt) + d[1:19]
        qvel[e, :] = d[19:43]
        k[e] += 1
        used.append(d)
    env.set_state(qpos, qvel, qw)
    return np.array(used)


def _assert_same_step(ea, eb, ra, rb, what):
    torch.cuda.synchronize()
    assert torch.equal(ra[0], rb[0]), (what, "obs")
    assert torch.equal(ra[2], rb[2]), (what, "reward")
    assert torch.equal(ra[3], rb[3]), (what, "done")
    assert torch.equal(ra[4]["time_outs"], rb[4]["time_outs"]), (what, "time_outs")
    _assert_same_state(ea, eb, what)


def _assert_same_state(ea, eb, what=""):
    for name, x, y in zip(("qpos", "qvel", "qacc_warmstart"), ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name}")


def _lock_step(ea, eb, N, npdt, steps=K):
    """Env A with the feature on, env B with it off and the test's host edits: reset_idx, then `steps` steps of one action stream.
    Returns (the test's reset counts, every edit's offsets, the steps at which each env reset)."""
    k = np.zeros(N, np.int64)
    _start(ea)
    _start(eb)
    edits = [_host_edit(eb, range(N), k, npdt)]
    _assert_same_state(ea, eb, "after reset_idx")
    acts = _actions(steps, N)
    when = [[] for _ in range(N)]
    for s in range(steps):
        ra, rb = ea.step(acts[s]), eb.step(acts[s])
        ids = np.nonzero(rb[3].cpu().numpy() > 0)[0]
        for e in ids:
            when[e].append(s)
        if len(ids):
            edits.append(_host_edit(eb, ids, k, npdt))
        _assert_same_step(ea, eb, ra, rb, f"step {s}")
    return k, edits, when


# ------------------------------------------------------------------------------------------------ 1. a reset draw = a host edit
@pytest.mark.parametrize("N,dtype", [(63, torch.float32), (1, torch.float32), (63, torch.float64)])
def test_a_reset_draw_equals_a_host_edit_of_the_state(N, dtype):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    ea, eb = _env(N, dtype, RANGES), _env(N, dtype)
    k, edits, when = _lock_step(ea, eb, N, npdt)
    on, ranges, counts = ea.reset_noise_state()
    assert on and np.array_equal(ranges, np.array(RANGES)) and np.array_equal(counts, k)
    off, zeros, none = eb.reset_noise_state()
    assert not off and not zeros.any() and not none.any()
    # the schedule of the module's docstring happened
    assert all(len(w) >= 2 for w in when), when
    if N > 1:
        pairs = [(set(when[2 * w]), set(when[2 * w + 1])) for w in range(N // 2)]
        assert any(a & b for a, b in pairs) and any(a - b for a, b in pairs) and any(b - a for a, b in pairs)
        assert 4 in when[6] and 9 in when[6]
    # the edits were edits: every draw moves its word, and two resets of one env differ
    first = edits[0]
    assert (np.abs(first) > 0).mean() > 0.99 and np.abs(first[:, 1:19]).max() > 0.05
    second = np.concatenate(edits[1:])
    assert not np.array_equal(first[0], second[0]) and len({e.tobytes() for ed in edits for e in ed}) == int(k.sum())
    for e in (ea, eb):
        e.close()


def test_lock_step_holds_with_pushes_and_latency_on_at_the_same_time():
    """Pushes every 3 steps and per-env actuation latency on both sides: a push of step t lands behind the reset draw of step t - 1 in
    qvel[0:2], and the action history is not the reset's business."""
    N = 63
    ea, eb = _env(N, ranges=RANGES, push=True), _env(N, push=True)
    for e in (ea, eb):
        e.draw_action_latency(0, 4)
    k, _, _ = _lock_step(ea, eb, N, np.float32)
    assert np.array_equal(ea.reset_noise_state()[2], k) and ea.push_state() == eb.push_state() == (3, 0.5, K)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 2. K-step launches = the per-step path
def _started(N, ranges, n, **kw):
    envs = [_env(N, ranges=ranges, **kw) for _ in range(n)]
    for e in envs:
        _start(e)
        _first_step(e)
    return envs


@pytest.mark.parametrize("N", [63, 130])
def test_tape_equals_the_per_step_path_and_two_launches_equal_one(N):
    """step_tape(K = 10) against 10 x step(), feature on in both: the three records row by row, the env afterwards, the reset counts, the
    books; tapes of 5 + 5 steps equal the 10-step one (envs 0, 1, 8, 9, ... reset at each launch's last step); and the run differs from
    the same run with the feature off."""
    ea, eb, ec = _started(N, RANGES, 3)
    (eo,) = _started(N, None, 1)
    acts = _actions(K, N)
    ep_idx = _ep_idx(ea)
    ba, bb, bc = (_books(N, ep_idx.numel()) for _ in range(3))
    rec, rec2, rec0 = _records(K, N), _records(K, N), _records(K, N)
    k0 = eb.reset_noise_state()[2]                            # reset_idx and the first step's resets
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
    ka, kb, kc = (e.reset_noise_state()[2] for e in (ea, eb, ec))
    assert np.array_equal(ka, kb) and np.array_equal(kc, kb)
    resets = per_step["done"].sum(dim=0).cpu().numpy()
    assert np.array_equal(kb, k0 + resets) and resets.min() >= 2 and k0.min() >= 1
    assert bool(per_step["done"][4].any()) and bool(per_step["done"][K - 1].any())       # resets at a launch's last step
    assert not torch.equal(rec["obs"], rec0["obs"])
    for e in (ea, eb, ec, eo):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
def test_play_equals_the_per_step_path_and_two_launches_equal_one(N):
    """policy_play(10) against 10 x [policy_act, step()], as test_gpu_play.py compares them, feature on in both; 5 + 5 equals 10."""
    ac, fu = _networks()
    ea, eb, ec = _started(N, RANGES, 3)
    (eo,) = _started(N, None, 1)
    it = torch.tensor([4], dtype=torch.int64, device=DEV)
    ep_idx = _ep_idx(ea)
    ba, bb, bc = (_books(N, ep_idx.numel()) for _ in range(3))
    oa = ea.policy_play(K, fu.flat, seed=77, iter_dev=it, stats=_stats(ba, ep_idx))
    ob, _ = _play_step_by_step(eb, fu, K, False, 77, it, bb, ep_idx)
    for _ in range(2):
        oc = ec.policy_play(5, fu.flat, seed=77, iter_dev=it, stats=_stats(bc, ep_idx))
    oo = eo.policy_play(K, fu.flat, seed=77, iter_dev=it)
    _assert_same_env(ea, eb, oa, ob)
    _assert_same_env(ec, eb, oc, ob)
    _assert_same_books(ba, bb)
    _assert_same_books(bc, bb)
    ka, kb, kc = (e.reset_noise_state()[2] for e in (ea, eb, ec))
    assert np.array_equal(ka, kb) and np.array_equal(kc, kb) and kb.min() >= 3
    assert not torch.equal(oa, oo)
    for e in (ea, eb, ec, eo):
        e.close()


@pytest.mark.parametrize("N", [63, 130])
def test_rollout_equals_the_per_step_path(N):
    """policy_rollout against [policy_act, step(), nm_ppo_record] per step, feature on in both: every storage row, the env afterwards,
    the reset counts, the books. nm_rollout refuses more steps than an episode has (an env may time out once per rollout), and an episode
    has 4 steps here: the 10 steps are launches of 4, 4 and 2 steps - consecutive launches, with resets at a launch's last step."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    gamma = 0.99
    ac, fu = _networks()
    ea, eb = _started(N, RANGES, 2)
    (eo,) = _started(N, None, 1)
    ep_idx = _ep_idx(ea)
    ba, bb, bo = (_books(N, ep_idx.numel()) for _ in range(3))
    o = eb.get_observations()
    differs = False
    for j, T in enumerate((4, 4, 2)):
        it = torch.tensor([3 + j], dtype=torch.int64, device=DEV)
        sa, sb, so = (_storage(N, T) for _ in range(3))
        oa = ea.policy_rollout(T, fu.flat, 99, it, sa, gamma, ba["cur_ret"], ba["cur_len"], ba["fin"], ep=(ep_idx, ba["ep_acc"]))
        eo.policy_rollout(T, fu.flat, 99, it, so, gamma, bo["cur_ret"], bo["cur_len"], bo["fin"], ep=(ep_idx, bo["ep_acc"]))
        for s in range(T):
            act = eb.policy_act(fu.flat, o, 99, it, s, sb)
            o, _, rew, done, infos = eb.step(act)
            _record(L, eb, sb, s, gamma, bb["cur_ret"], bb["cur_len"], bb["fin"], ep_idx, bb["ep_acc"])
        torch.cuda.synchronize()
        for name in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), (j, name)
        _assert_same_env(ea, eb, oa, o)
        assert torch.equal(ba["cur_ret"], bb["cur_ret"]) and torch.equal(ba["cur_len"], bb["cur_len"])
        assert np.array_equal(ea.reset_noise_state()[2], eb.reset_noise_state()[2])
        differs = differs or not torch.equal(sa.observations, so.observations)
    assert differs and ea.reset_noise_state()[2].min() >= 3
    for e in (ea, eb, eo):
        e.close()


# ------------------------------------------------------------------------------------------------ 3. zero ranges = off
def test_zero_ranges_equal_off_bit_for_bit_and_off_keeps_the_counts():
    """Per-step and tape, N = 63: env Z with ten zeros against env O that never heard of the feature; then a third env that ran with real
    ranges is switched off - set_reset_noise(None) keeps its counts - and, from the same state, equals O again."""
    N = 63
    zeros = ((0.0, 0.0),) * 5
    ez, eo = _env(N, ranges=zeros), _env(N)
    for e in (ez, eo):
        _start(e)
    _assert_same_state(ez, eo, "after reset_idx")
    acts = _actions(2 * K, N)
    for s in range(K):
        _assert_same_step(ez, eo, ez.step(acts[s]), eo.step(acts[s]), f"zeros, step {s}")
    rz, ro = _records(K, N), _records(K, N)
    oz, oo = ez.step_tape(acts[K:].contiguous(), record=rz), eo.step_tape(acts[K:].contiguous(), record=ro)
    torch.cuda.synchronize()
    for n in rz:
        assert torch.equal(rz[n], ro[n]), n
    _assert_same_env(ez, eo, oz, oo)
    kz = ez.reset_noise_state()[2]
    assert kz.min() >= 5 and not eo.reset_noise_state()[2].any()           # Z counted its resets all the same
    # off after on: two envs with the same history under real ranges; one is switched off, the other to ten zeros (= off, as shown above)
    q0 = _env(1)
    q0.reset_idx(None)
    qpos0 = q0.get_state()[0][0].copy()
    q0.close()
    en, et = _env(N, ranges=RANGES), _env(N, ranges=RANGES)
    for e in (en, et):
        _start(e)
        for s in range(3):
            e.step(acts[s])
    before = en.reset_noise_state()[2].copy()
    assert before.min() >= 1 and before.max() >= 2
    en.set_reset_noise(None)
    et.set_reset_noise(zeros)
    on, ranges, counts = en.reset_noise_state()
    assert not on and not ranges.any() and np.array_equal(counts, before)      # set_reset_noise(None) keeps the counts
    seen = 0
    for s in range(3, 3 + K):
        rn, rt = en.step(acts[s]), et.step(acts[s])
        _assert_same_step(en, et, rn, rt, f"off after on, step {s}")
        d = rn[3].cpu().numpy() > 0
        if d.any():                                                          # a reset row is qpos0 / zero velocity again
            q, v, _ = en.get_state()
            assert (q[d] == qpos0).all() and not v[d].any()
            seen += int(d.sum())
    assert seen >= N and np.array_equal(en.reset_noise_state()[2], before)
    # and on again with installed counts: the next reset of env 5 is draw before[5] + 7
    en.set_reset_noise(RANGES, counts=before + 7)
    assert np.array_equal(en.reset_noise_state()[2], before + 7)
    en.reset_idx([5])
    q, v, _ = en.get_state()
    d = restated_offsets(RANGES, SEED, 5, int(before[5]) + 7, np.float32)
    np.testing.assert_array_equal(v[5], d[19:43].astype(np.float64))
    np.testing.assert_array_equal(q[5, 7:25], (qpos0[7:25].astype(np.float32) + d[1:19]).astype(np.float64))
    assert en.reset_noise_state()[2][5] == before[5] + 8 and (en.reset_noise_state()[2][:5] == before[:5] + 7).all()
    for e in (ez, eo, en, et):
        e.close()


# ------------------------------------------------------------------------------------------------ 4. sharding
def test_reset_draws_do_not_depend_on_sharding():
    """One 63-env object against two objects of 32 and 31 envs with env_id_offset 0 and 32: reset_idx, 10 x step(), then a 10-step tape,
    row for row."""
    N, cut = 63, 32
    whole = _env(N, ranges=RANGES)
    parts = [_env(cut, ranges=RANGES, offset=0), _env(N - cut, ranges=RANGES, offset=cut)]
    _start(whole)
    for p, off in zip(parts, (0, cut)):
        _start(p, off)
    sl = [slice(0, cut), slice(cut, N)]

    def same_state(what):
        for x, ys in zip(whole.get_state(), zip(*[p.get_state() for p in parts])):
            np.testing.assert_array_equal(x, np.concatenate(ys), err_msg=what)
        assert np.array_equal(whole.reset_noise_state()[2], np.concatenate([p.reset_noise_state()[2] for p in parts])), what

    same_state("after reset_idx")
    acts = _actions(2 * K, N)
    for s in range(K):
        rw = whole.step(acts[s])
        rp = [p.step(acts[s, i].contiguous()) for p, i in zip(parts, sl)]
        torch.cuda.synchronize()
        for j in (0, 2, 3):
            assert torch.equal(rw[j], torch.cat([r[j] for r in rp])), (s, j)
        assert torch.equal(rw[4]["time_outs"], torch.cat([r[4]["time_outs"] for r in rp])), s
        same_state(f"step {s}")
    rec = _records(K, N)
    whole.step_tape(acts[K:].contiguous(), record=rec)
    recs = [_records(K, p.num_envs) for p in parts]
    for p, i, r in zip(parts, sl, recs):
        p.step_tape(acts[K:, i].contiguous(), record=r)
    torch.cuda.synchronize()
    for n in ("obs", "rew", "done"):
        assert torch.equal(rec[n], torch.cat([r[n] for r in recs], dim=1)), n
    same_state("after the tape")
    assert whole.reset_noise_state()[2].min() >= 5
    for e in [whole] + parts:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. refusals with an env
def test_the_env_refuses_bad_ranges_and_changes_nothing():
    from nightmare_rl_amd import _lib
    env = _env(4, ranges=RANGES)
    bad = [list(r) for r in RANGES]
    bad[2] = [0.4, -0.4]
    with pytest.raises(_lib.NightmareHipError, match="lo > hi for base_lin_vel"):
        env.set_reset_noise(bad)
    bad[2] = [0.0, 1e39]                                                     # not finite in the env's float32
    with pytest.raises(_lib.NightmareHipError, match="base_lin_vel"):
        env.set_reset_noise(bad)
    with pytest.raises(ValueError, match="five"):
        env.set_reset_noise([(0, 1)] * 4)
    with pytest.raises(ValueError, match="num_envs"):
        env.set_reset_noise(RANGES, counts=[1, 2, 3])
    on, ranges, counts = env.reset_noise_state()
    assert on and np.array_equal(ranges, np.array(RANGES)) and not counts.any()
    assert env._L.nm_get_reset_noise(env._h, None, None, None) == 0            # every out pointer is optional
    env.close()
