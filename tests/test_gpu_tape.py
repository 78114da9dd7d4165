"""K-step action-tape stepping (nm_step_tape / NightmareV3Env.step_tape) and the K-tick gait tape (nm_nik_tape / EngineNode.tape) against
their per-step paths - one nm_step launch per action row, one nm_nik_update launch per tick - BIT FOR BIT. The only tolerances are the
project's for sums that go through float atomics (fin3, ep_acc: atol 1e-3, rtol 1e-5, count exact; extras['episode']: atol 1e-6, rtol 1e-4)."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import make_env
from test_gpu_play import _assert_same_records, _books, _env, _ep_idx, _pickles, _spread_episode_lengths, _stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tape(K, N, seed=17):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(K, N, 18, generator=g) * 2 - 1).to(DEV).contiguous()


def _records(K, N):
    return dict(obs=torch.full((K, N, 66), float("nan"), device=DEV), rew=torch.full((K, N), float("nan"), device=DEV),
                done=torch.full((K, N), 255, dtype=torch.uint8, device=DEV))


def _step_by_step(env, actions, b, ep_idx):
    """K x env.step(actions[t]) with the bookkeeping as plain fp32 tensor arithmetic in step order (test_gpu_play._step_by_step without the
    policy). Returns (last observation, number of time-outs per env, what every step returned: obs [K,N,66], rew [K,N], done [K,N] u8)."""
    n_to = torch.zeros(env.num_envs, device=DEV)
    obs, rews, dones = [], [], []
    o = env.get_observations()
    for s in range(actions.shape[0]):
        o, _, rew, done, _ = env.step(actions[s])
        obs.append(o.clone()); rews.append(rew.clone()); dones.append(done.to(torch.uint8))
        d = done > 0
        b["cur_ret"] += rew
        b["cur_len"] += 1
        b["fin"] += torch.stack([(b["cur_ret"] * d).sum(), (b["cur_len"] * d).sum(), d.float().sum()])
        b["ret_sum"] += torch.where(d, b["cur_ret"], torch.zeros_like(rew))
        b["ret_cnt"] += d.float()
        if bool(d.any()):                    # a step with a reset refreshes the time-out flags of that step (env.py:369)
            n_to += env.time_out_buf * d.float()
        b["cur_ret"][d] = 0
        b["cur_len"][d] = 0
        b["ep_acc"] += env._ep_stats.index_select(0, ep_idx.long())
    return o, n_to, dict(obs=torch.stack(obs), rew=torch.stack(rews), done=torch.stack(dones))


def _assert_same_env(ea, eb, oa, ob):
    torch.cuda.synchronize()
    assert torch.equal(oa, ob) and torch.equal(ea.rew_buf, eb.rew_buf) and torch.equal(ea.reset_buf, eb.reset_buf)
    assert torch.equal(ea.obs_buf, eb.obs_buf)
    assert torch.equal(ea.episode_length_buf, eb.episode_length_buf) and torch.equal(ea.time_out_buf, eb.time_out_buf)
    for x, y in zip(ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y)
    ba, bb = ea.get_buffers(), eb.get_buffers()
    for k in ba:
        np.testing.assert_array_equal(ba[k], bb[k], err_msg=k)
    for x, y in zip(ea.get_feet_state(), eb.get_feet_state()):
        np.testing.assert_array_equal(x, y)
    assert ea.counters() == eb.counters() and ea.common_step_counter == eb.common_step_counter
    assert ("time_outs" in ea.extras) == ("time_outs" in eb.extras)


def _assert_same_books(a, b):
    for k in ("cur_ret", "cur_len", "ret_sum", "ret_cnt"):
        assert torch.equal(a[k], b[k]), k
    print("fin", a["fin"].tolist(), b["fin"].tolist(), "ep_acc max diff", float((a["ep_acc"] - b["ep_acc"]).abs().max()))
    torch.testing.assert_close(a["fin"], b["fin"], atol=1e-3, rtol=1e-5)                 # float atomics: order of the additions differs
    assert a["fin"][2] == b["fin"][2]
    torch.testing.assert_close(a["ep_acc"], b["ep_acc"], atol=1e-3, rtol=1e-5)


def _upside_down(env, ids):
    qpos, qvel, qw = env.get_state()
    qpos[ids, 3:7] = (0.0, 1.0, 0.0, 0.0)
    env.set_state(qpos, qvel, qw)


# ------------------------------------------------------------------------------------------------ 1. tape vs step by step
CASES = [  # N, K, noise, episode_length_s
    (1, 1, False, None),            # a wave with one env, the shortest launch
    (63, 90, False, None),          # odd N, a half-empty last wave; two envs start upside down
    (130, 40, True, None),          # 65 waves: the XCD mapping's remainder; observation noise
    (64, 70, False, 0.5),           # 32-step episodes: every env times out at least twice inside the launch
]


@pytest.mark.parametrize("N,K,noise,ep_s", CASES)
def test_tape_equals_the_step_by_step_path_bit_for_bit(N, K, noise, ep_s):
    """step_tape(actions) with all three records and all stats against K x env.step(actions[t]) from the same start: every record row
    against what the step returned, the final observation / reward / reset / episode-length / time-out buffers, state, buffers, feet
    state, counters, common_step_counter; cur_ret, cur_len, ret_sum, ret_cnt exactly; fin3 / ep_acc / extras['episode'] to the atomic
    tolerances. Then three plain step() calls stay equal on both sides."""
    envs = [_env(N, noise=noise, episode_length_s=ep_s) for _ in range(2)]
    for e in envs:
        e.reset()
        if ep_s is None:
            _spread_episode_lengths(e, N)
        if (N, K) == (63, 90):
            _upside_down(e, [3, 4])
    if ep_s is not None:
        assert K > 2 * int(envs[0].max_episode_length)
    actions = _tape(K, N)
    ep_idx = _ep_idx(envs[0])
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    rec = _records(K, N)
    before = envs[0].get_observations()
    keep = before.clone()
    oa = envs[0].step_tape(actions, record=rec, stats=_stats(ba, ep_idx))
    ob, n_to, per_step = _step_by_step(envs[1], actions, bb, ep_idx)
    torch.cuda.synchronize()
    assert torch.equal(before, keep)                          # the tensor handed out before stays untouched
    for k in ("obs", "rew", "done"):
        assert torch.equal(rec[k], per_step[k]), k
    if (N, K) == (63, 90):
        assert int(rec["done"][0, 3]) == 1 and int(rec["done"][0, 4]) == 1        # terminated by the tilt rule inside the tape
    if ep_s is not None:
        print("time-outs per env: min", float(n_to.min()), "max", float(n_to.max()))
        assert float(n_to.min()) >= 2, "every env must time out at least twice within the launch"
    _assert_same_env(envs[0], envs[1], oa, ob)
    _assert_same_books(ba, bb)
    torch.testing.assert_close(envs[0]._ep_stats, envs[1]._ep_stats, atol=1e-6, rtol=1e-4)
    a = torch.rand(N, 18, device=DEV) * 2 - 1
    for _ in range(3):
        ra, rb = envs[0].step(a), envs[1].step(a)
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[2], rb[2]) and torch.equal(ra[3], rb[3])
        assert torch.equal(ra[4]["time_outs"], rb[4]["time_outs"])
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. two tapes = one tape = per step
def test_tape_in_two_launches_equals_one_launch_and_the_per_step_run(tmp_path):
    """step_tape(K1) then step_tape(K2) == step_tape(K1 + K2) on the concatenated tape (K1 odd) == K1 + K2 step() calls, with the state
    log on and the logged env timing out inside: env, books, the pickle files written and the pending records."""
    N, K1, K2 = 32, 33, 40
    dirs = [str(tmp_path / n) for n in "abc"]
    envs = [_env(N, record=True, log_dir=d) for d in dirs]
    for e in envs:
        e.reset()
        _spread_episode_lengths(e, N)
        e.episode_length_buf[0] = int(e.max_episode_length) - 20
    actions = _tape(K1 + K2, N)
    ep_idx = _ep_idx(envs[0])
    books = [_books(N, ep_idx.numel()) for _ in envs]
    envs[0].step_tape(actions[:K1], stats=_stats(books[0], ep_idx))
    oa = envs[0].step_tape(actions[K1:], stats=_stats(books[0], ep_idx))
    ob = envs[1].step_tape(actions, stats=_stats(books[1], ep_idx))
    oc, _, per_step = _step_by_step(envs[2], actions, books[2], ep_idx)
    assert int(per_step["done"][:, 0].sum()) >= 1
    for k in (1, 2):
        _assert_same_env(envs[0], envs[k], oa, (ob, oc)[k - 1])
        _assert_same_books(books[0], books[k])
    files = [_pickles(d) for d in dirs]
    assert len(files[0]) == len(files[1]) == len(files[2]) >= 1
    for k in (1, 2):
        for x, y in zip(files[0], files[k]):
            _assert_same_records(x, y)
        _assert_same_records(envs[0].recorded_states, envs[k].recorded_states)
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. records off = records on
def test_tape_without_records_equals_the_tape_with_records():
    N, K = 66, 45
    envs = [_env(N) for _ in range(2)]
    for e in envs:
        e.reset()
        _spread_episode_lengths(e, N)
    actions = _tape(K, N)
    ep_idx = _ep_idx(envs[0])
    ba, bb = _books(N, ep_idx.numel()), _books(N, ep_idx.numel())
    oa = envs[0].step_tape(actions, stats=_stats(ba, ep_idx))
    ob = envs[1].step_tape(actions, record=_records(K, N), stats=_stats(bb, ep_idx))
    _assert_same_env(envs[0], envs[1], oa, ob)
    _assert_same_books(ba, bb)
    # and with no stats at all the env ends up the same
    e3 = _env(N)
    e3.reset()
    _spread_episode_lengths(e3, N)
    oc = e3.step_tape(actions)
    _assert_same_env(envs[0], e3, oa, oc)
    for e in envs + [e3]:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_tape_refuses_what_it_cannot_do():
    from nightmare_rl_amd import _lib
    env64 = make_env(8, dtype=torch.float64)
    env64.reset()
    with pytest.raises(_lib.NightmareHipError, match="fp32"):
        env64.step_tape(torch.zeros(4, 8, 18, device=DEV))
    env = make_env(8)
    env.reset()
    ok = torch.zeros(4, 8, 18, device=DEV)
    bad = [torch.zeros(4, 8, 17, device=DEV), torch.zeros(4, 7, 18, device=DEV), torch.zeros(8, 18, device=DEV),       # shape
           torch.zeros(4, 8, 18, device=DEV, dtype=torch.float64), torch.zeros(4, 8, 18),                               # dtype, device
           torch.zeros(4, 8, 36, device=DEV)[:, :, ::2], torch.zeros(0, 8, 18, device=DEV)]                             # non-contiguous, K = 0
    for t in bad:
        with pytest.raises(ValueError):
            env.step_tape(t)
    with pytest.raises(ValueError, match="unknown"):
        env.step_tape(ok, record=dict(observations=torch.zeros(4, 8, 66, device=DEV)))
    with pytest.raises(ValueError, match="unknown"):
        env.step_tape(ok, stats=dict(returns=torch.zeros(8, device=DEV)))
    with pytest.raises(ValueError):
        env.step_tape(ok, record=dict(done=torch.zeros(4, 8, device=DEV)))                  # done is uint8
    with pytest.raises(ValueError):
        env.step_tape(ok, record=dict(obs=torch.zeros(3, 8, 66, device=DEV)))               # one row per step
    with pytest.raises(ValueError, match="pairs"):
        env.step_tape(ok, stats=dict(cur_ret=torch.zeros(8, device=DEV)))
    count = env.common_step_counter
    env.step_tape(ok)                                                                        # and the well-formed call goes through
    assert env.common_step_counter == count + 4
    env.close(); env64.close()


# ------------------------------------------------------------------------------------------------ 5. gait tape vs per tick
def _same_engine_state(a, b, where):
    sa, sb = a.get_state(), b.get_state()
    for k in ("fsm", "pose", "gait_step_state"):
        assert np.array_equal(sa[k], sb[k]), (where, k)


def test_gait_tape_equals_the_per_tick_engine_bit_for_bit():
    """The population of test_ik_table_through_the_kernel_matches_oracle_batch (37 engines, 420 ticks at 62.5 fps, commands redrawn every
    40 ticks, three engines reset at tick 250, some asleep or standing from tick 300): EngineNode(float64).tape in chunks that end at
    those events against one update(time_s=tick * dt) per tick - all 420 x 37 x 18 float64 targets and the engine state at every chunk
    boundary, exactly."""
    from nightmare_rl_amd import nikengine as nk
    N, T, fps = 37, 420, 62.5
    dt = 1.0 / fps
    rng = np.random.default_rng(5)
    nk.config.ENGINE_FPS = fps
    ea, eb = nk.EngineNode(N, dtype=torch.float64), nk.EngineNode(N, dtype=torch.float64)
    lin = rng.uniform(-0.25, 0.25, N).astype(np.float32)
    ang = rng.uniform(-1.2, 1.2, N).astype(np.float32)
    awake, walk = np.ones(N, bool), np.ones(N, bool)
    bounds = sorted(set(range(0, T + 1, 40)) | {250, 300, T})
    assert {240, 250, 280, 300, 320} <= set(bounds)
    seen = set()
    got, exp = [], []
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        if b0 % 40 == 0:
            lin = rng.uniform(-0.25, 0.25, N).astype(np.float32)
            ang = rng.uniform(-1.2, 1.2, N).astype(np.float32)
        if b0 == 300:
            awake[::5] = False
            walk[1::5] = False
        if b0 == 250:
            ids = np.array([3, 11, 36])
            ea.reset(ids)
            eb.reset(ids)
        args = (torch.as_tensor(lin).to(DEV), torch.as_tensor(ang).to(DEV), torch.as_tensor(awake), torch.as_tensor(walk))
        out = ea.tape(*args, steps=b1 - b0, tick0=b0, dt=dt)
        assert out.dtype == torch.float64 and tuple(out.shape) == (b1 - b0, N, 18)
        got.append(out.cpu().numpy())
        for t in range(b0, b1):
            exp.append(eb.update(*args, time_s=t * dt).cpu().numpy())
            seen |= set(eb.get_state()["fsm"].tolist())
        _same_engine_state(ea, eb, b1)
    got, exp = np.concatenate(got), np.stack(exp)
    assert got.shape == exp.shape == (T, N, 18) and np.isfinite(exp).all()
    assert np.array_equal(got, exp), np.abs(got - exp).max()
    assert {0, 1, 2, 5, 6} <= seen
    # one chunk with the ripple gait on env 0 and wave on env 1 (long enough to get up and walk several gait cycles)
    ea, eb = nk.EngineNode(2, dtype=torch.float64), nk.EngineNode(2, dtype=torch.float64)
    for e in (ea, eb):
        e.set_gait("ripple", [0])
        e.set_gait("wave", [1])
    lin2, ang2 = torch.full((2,), 0.1, dtype=torch.float64, device=DEV), torch.full((2,), 0.3, dtype=torch.float64, device=DEV)
    out = ea.tape(lin2, ang2, steps=T, tick0=0, dt=dt).cpu().numpy()
    ref = np.stack([eb.update(lin2, ang2, time_s=t * dt).cpu().numpy() for t in range(T)])
    assert np.array_equal(out, ref), np.abs(out - ref).max()
    _same_engine_state(ea, eb, "gaits")
    assert (ea.get_state()["fsm"] == 6).all()
    with pytest.raises(ValueError):
        ea.tape(lin2, ang2, steps=0, tick0=0, dt=dt)
    nk.config.ENGINE_FPS = 51.0


# ------------------------------------------------------------------------------------------------ 6. the servo stage
def _servo_f32(goals, q, rate, default_pos3, action_scale):
    """custom_play.py:72 and the inverse action mapping restated in numpy float32, every operation rounded on its own: sub, clip, add, add,
    multiply by float32(1 / action_scale). goals [K,N,18] f32, q [N,18] f32 (updated in place). Returns the [K,N,18] actions."""
    rate, inv = np.float32(rate), np.float32(1.0 / action_scale)
    dp = np.tile(np.asarray(default_pos3, np.float32), 6)
    out = np.empty_like(goals)
    for t in range(goals.shape[0]):
        d = goals[t] - q
        q += np.clip(d, -rate, rate)
        out[t] = (q + dp) * inv
    assert out.dtype == np.float32
    return out


def test_servo_stage_equals_its_numpy_float32_restatement():
    from nightmare_rl_amd import nikengine as nk
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    N, K1, K2, fps = 37, 150, 170, 62.5
    dt = 1.0 / fps
    nk.config.ENGINE_FPS = fps
    rng = np.random.default_rng(9)
    lin = torch.as_tensor(rng.uniform(-0.25, 0.25, N)).to(DEV)
    ang = torch.as_tensor(rng.uniform(-1.2, 1.2, N)).to(DEV)
    dp3 = [float(x) for x in NightmareV3Config().control.default_pos[:3]]
    servo = dict(targets=torch.zeros(N, 18, device=DEV), action_rate=0.08, default_pos=dp3, action_scale=0.2)
    ea, eb = nk.EngineNode(N), nk.EngineNode(N)
    a1 = ea.tape(lin, ang, steps=K1, tick0=0, dt=dt, servo=servo)
    a2 = ea.tape(lin, ang, steps=K2, tick0=K1, dt=dt, servo=servo)          # the limiter's memory carries over
    assert a1.dtype == torch.float32 and tuple(a2.shape) == (K2, N, 18)
    goals = np.stack([eb.update(lin, ang, time_s=t * dt).cpu().numpy() for t in range(K1 + K2)])
    assert goals.dtype == np.float32
    q = np.zeros((N, 18), np.float32)
    want = _servo_f32(goals, q, 0.08, dp3, 0.2)
    got = torch.cat([a1, a2]).cpu().numpy()
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert np.array_equal(servo["targets"].cpu().numpy(), q)
    assert (eb.get_state()["fsm"] == 6).all()                                  # the comparison reached walking
    with pytest.raises(ValueError):
        ea.tape(lin, ang, steps=2, tick0=0, dt=dt, servo=dict(targets=servo["targets"]))
    nk.config.ENGINE_FPS = 51.0


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_two_launch_custom_play_walks_the_robot_and_equals_its_per_step_loop():
    """scripts/custom_play.py play(one_launch=True): the bounds of test_gait_engine_walks_the_simulated_robot, and the final qpos of the
    same run done per step here - update, the servo arithmetic of the test above in fp32 tensor operations (each rounded on its own),
    env.step - exactly."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from custom_play import play
    from nightmare_rl_amd import nikengine as nk
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    from nightmare_rl_amd.envs.nightmare_v3_env import NightmareV3Env
    N, seconds, lin, rate = 32, 10.0, 0.05, 0.08
    r = play(num_envs=N, seconds=seconds, lin=lin, ang=0.0, one_launch=True, launch_steps=100)
    dist = np.linalg.norm(r["displacement"][:, :2], axis=1)
    assert r["falls"] == 0
    assert (r["fsm"] == 6).all()
    assert 0.07 < r["height"].min() and r["height"].max() < 0.13, (r["height"].min(), r["height"].max())
    assert 0.6 < dist.min() and dist.max() < 1.5, (dist.min(), dist.max())
    # the same run, one launch per tick and per step
    cfg = NightmareV3Config()
    cfg.env.num_envs = N
    cfg.env.episode_length_s = 1e6
    env = NightmareV3Env(cfg, device=DEV, seed=0)
    env.reset()
    nk.config.ENGINE_FPS = 1.0 / env.dt
    eng = nk.EngineNode(N, device=DEV)
    lin_t = torch.full((N,), lin, device=DEV, dtype=torch.float64)
    ang_t = torch.zeros(N, device=DEV, dtype=torch.float64)
    q = torch.zeros(N, 18, device=DEV)
    dp = torch.tensor([float(np.float32(x)) for x in env.default_dof_pos[:3]] * 6, device=DEV)
    inv = float(np.float32(1.0 / float(cfg.control.action_scale)))
    for i in range(int(seconds / env.dt)):
        goal = eng.update(lin_t, ang_t, time_s=i * env.dt)
        q = q + torch.clamp(goal - q, -rate, rate)
        env.step((q + dp) * inv)
    qpos = env.get_state()[0]
    nk.config.ENGINE_FPS = 51.0
    assert np.array_equal(r["qpos"], qpos), np.abs(r["qpos"] - qpos).max()
    env.close()
