"""The per-env sensor model (observation latency and bias; csrc/nm_sensor.h) on the device: k_sensor behind step(), and nmr::step_sensor inside
the K-step launches (policy_rollout symmetric and privileged, policy_play, step_tape), against the numpy restatement of the model's three
rules (tests/sensor_np.py) and against each other. The model is a copy, one float32 add and a clamp: every comparison is equality.
N = 5 (an odd last wave) and N = 2, K = 12; episode lengths are staggered so that some envs reset inside the window and some do not."""
import numpy as np
import pytest
import torch

import sensor_np as sn
from test_gpu_parity import make_env
from test_gpu_rollout import _record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, NOBS = 12, 66
CLIP = np.float32(100.0)          # cfg.normalization.clip_observations of the shipped config


def _stagger(env):
    """Env 0 times out at step 3 of the window, env 2 (if there is one) at step 7; the others run through."""
    M = int(env.max_episode_length)
    b = 5 * torch.arange(env.num_envs, dtype=torch.int64, device=DEV)
    b[0] = M - 3
    if env.num_envs > 2:
        b[2] = M - 7
    env.episode_length_buf = b


def _start(N, model=None, seed=11, priv=False, kind=False, offset=0):
    if priv:
        from test_gpu_privileged_obs import _env
        env = _env(N, seed=seed)
    else:
        env = make_env(N, seed=seed, env_id_offset=offset)
    if kind:                       # one per-env kind on: a higher level's instantiation of the K-step kernels
        env.set_env_params(mu=np.linspace(0.6, 1.1, N))
    env.reset()
    _stagger(env)
    if model is not None:          # after reset(), whose zero-action step would otherwise be the history's first entry
        env.set_sensor_model(*model)
    return env


def _tape(N, seed=17):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((K, N, 18), generator=g) * 2 - 1).to(DEV)


def _resets_inside(done):
    d = np.asarray(done, bool)
    assert d[:-1].any(axis=0).any() and not d.any(axis=0).all(), d.any(axis=0)      # at least one env resets inside the window, at least one never


def _same_state(a, b):
    (ra, ca), (rb, cb) = a.sensor_state(), b.sensor_state()
    np.testing.assert_array_equal(ca, cb)
    np.testing.assert_array_equal(ra, rb)


# ------------------------------------------------------------------------------------------------ 3. the tape path against the restatement
@pytest.mark.parametrize("N", [5, 2])
def test_tape_records_the_restated_rows_in_every_stepping_path(N):
    tape, model = _tape(N), sn.model(N, 1)
    rec = lambda: dict(obs=torch.zeros((K, N, NOBS), device=DEV), done=torch.zeros((K, N), dtype=torch.uint8, device=DEV))
    A, ra = _start(N), rec()                       # the model off: true rows and dones
    A.step_tape(tape, record=ra)
    y, done = ra["obs"].cpu().numpy(), ra["done"].cpu().numpy() > 0
    _resets_inside(done)
    want, want_count = sn.sensed(y, done, *model, CLIP)
    assert (np.abs(want) == CLIP).any() and not np.array_equal(want, y)
    B, rb = _start(N, model), rec()                # one launch
    ob = B.step_tape(tape, record=rb)
    got = rb["obs"].cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    np.testing.assert_array_equal(got.view(np.uint32)[..., sn.PASS], y.view(np.uint32)[..., sn.PASS])
    assert torch.equal(rb["done"], ra["done"])
    assert torch.equal(B.true_observations(), ra["obs"][-1]) and torch.equal(ob, rb["obs"][-1]) and ob is B.get_observations()
    np.testing.assert_array_equal(B.sensor_state()[1], want_count)
    Cs = _start(N, model)                          # 12 calls of step()
    rows = torch.stack([Cs.step(tape[t])[0].clone() for t in range(K)])
    assert torch.equal(rows, rb["obs"]) and torch.equal(Cs.true_observations(), ra["obs"][-1])
    _same_state(Cs, B)
    D, rd = _start(N, model), rec()                # launches of 5 + 7
    D.step_tape(tape[:5].contiguous(), record={k: v[:5] for k, v in rd.items()})
    D.step_tape(tape[5:].contiguous(), record={k: v[5:] for k, v in rd.items()})
    assert torch.equal(rd["obs"], rb["obs"])
    _same_state(D, B)
    E = _start(N, model)                           # no observation record: the sensed row goes to the env's own buffer
    oe = E.step_tape(tape)
    assert torch.equal(oe, rb["obs"][-1]) and torch.equal(E.true_observations(), ra["obs"][-1])
    _same_state(E, B)
    state = A.get_state()
    for e in (A, B, Cs, D, E):
        for x, z in zip(e.get_state(), state):      # the physics never sees the model
            np.testing.assert_array_equal(x, z)
        e.close()


# ------------------------------------------------------------------------------------------------ 4. rollouts
def _nets(priv, activation):
    if priv:
        from test_gpu_privileged_rollout import _networks, _storage
    else:
        from test_gpu_play import _networks, _storage
    ac, fu = _networks(activation)
    return fu, _storage


def _rollout_pair(N, priv, activation, kind, model, modes=(True, False)):
    """One entry per mode. True: policy_rollout in one launch. False: K x [policy_act, step(), nm_ppo_record], keeping every step's true row and dones."""
    from nightmare_rl_amd import _lib
    L = _lib.load()
    fu, storage = _nets(priv, activation)
    it = torch.tensor([3], dtype=torch.int64, device=DEV)
    out = []
    for one_launch in modes:
        env = _start(N, model, priv=priv, kind=kind)
        ep_idx = torch.tensor([env._stat_names.index(k[4:]) for k in sorted(env.extras["episode"])], dtype=torch.int32, device=DEV)
        z = lambda n: torch.zeros(n, device=DEV)
        bk = dict(cur_ret=z(N), cur_len=z(N), fin=z(3), ep_acc=z(ep_idx.numel()))
        st, lv, truth = storage(N, K), torch.full((N,), float("nan"), device=DEV), []
        if one_launch:
            o = env.policy_rollout(K, fu.flat, 99, it, st, 0.99, bk["cur_ret"], bk["cur_len"], bk["fin"], ep=(ep_idx, bk["ep_acc"]), last_values=lv, activation=activation)
            rows = env.get_privileged_observations()
        else:
            o, rows, pcols = env.get_observations(), env.get_privileged_observations(), []
            for s in range(K):
                act = env.policy_act(fu.flat, rows if priv else o, 99, it, s, st, activation=activation)
                o, rows, _, _, _ = env.step(act)
                _record(L, env, st, s, 0.99, bk["cur_ret"], bk["cur_len"], bk["fin"], ep_idx, bk["ep_acc"])
                truth.append(env.true_observations())
                if priv:
                    pcols.append(rows[:, NOBS:].clone())
            tmp = storage(N, 1)
            env.policy_act(fu.flat, rows if priv else o, 99, it, 0, tmp, activation=activation)
            lv = tmp.values[0].view(-1).clone()
            if priv:
                st.pcols = torch.stack(pcols)
        torch.cuda.synchronize()
        out.append(dict(env=env, st=st, obs=o, rows=rows, lv=lv, bk=bk, truth=torch.stack(truth) if truth else None))
    return out


@pytest.mark.parametrize("N,priv,activation,kind", [(5, p, a, k) for p in (False, True) for a in ("elu", "tanh") for k in (False, True)] + [(2, False, "elu", False), (2, True, "elu", True)])
def test_one_launch_rollout_equals_step_by_step_with_the_model_on(N, priv, activation, kind):
    model = sn.model(N, 2)
    a, b = _rollout_pair(N, priv, activation, kind, model)
    names = ("observations", "actions", "actions_log_prob", "values", "rewards", "dones", "mu", "sigma") + (("privileged_observations",) if priv else ())
    for name in names:
        x, y = getattr(a["st"], name), getattr(b["st"], name)
        assert torch.equal(x, y), (name, (x != y).nonzero()[:6].tolist())
    assert torch.equal(a["obs"], b["obs"]) and torch.equal(a["lv"], b["lv"]) and torch.isfinite(a["lv"]).all()
    assert torch.equal(a["env"].true_observations(), b["env"].true_observations())
    assert torch.equal(a["bk"]["cur_ret"], b["bk"]["cur_ret"]) and torch.equal(a["bk"]["cur_len"], b["bk"]["cur_len"])
    _same_state(a["env"], b["env"])
    if priv:
        sa = a["st"]
        assert torch.equal(a["rows"], b["rows"]) and torch.equal(a["rows"][:, :NOBS], a["obs"])
        assert torch.equal(sa.privileged_observations[..., :NOBS], sa.observations)
        assert torch.equal(sa.privileged_observations[1:, :, NOBS:], b["st"].pcols[:-1]) and torch.equal(a["rows"][:, NOBS:], b["st"].pcols[-1])
    # the step-by-step run's sensed rows are the restatement of its own true rows and dones
    y, done = b["truth"].cpu().numpy(), b["st"].dones.squeeze(-1).cpu().numpy() > 0
    _resets_inside(done)
    want, want_count = sn.sensed(y, done, *model, CLIP)
    got = torch.cat([b["st"].observations[1:], b["obs"][None]]).cpu().numpy()         # row s + 1 of the storage is what step s returned
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    assert not np.array_equal(want, y)
    np.testing.assert_array_equal(b["env"].sensor_state()[1], want_count)
    a["env"].close(); b["env"].close()


# ------------------------------------------------------------------------------------------------ 5. play
@pytest.mark.parametrize("N", [5, 2])
def test_play_in_one_launch_equals_twelve_launches_of_one_step(N):
    from test_gpu_play import _networks
    _, fu = _networks()
    model = sn.model(N, 3)
    z = lambda n: torch.zeros(n, device=DEV)
    res = []
    for pieces in ([K], [1] * K):
        env = _start(N, model)
        stats = dict(ret_sum=z(N), ret_cnt=z(N), cur_ret=z(N), cur_len=z(N))
        for k in pieces:
            o = env.policy_play(k, fu.flat, seed=5, stats=stats)
        torch.cuda.synchronize()
        res.append((env, o.clone(), stats))
    (ea, oa, sa), (eb, ob, sb) = res
    assert torch.equal(oa, ob) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(ea.true_observations(), eb.true_observations()) and not torch.equal(ea.true_observations(), oa)
    assert float(sa["ret_cnt"].sum()) >= 1 and float(sa["ret_cnt"].min()) == 0        # an env reset inside the window, another did not
    _same_state(ea, eb)
    ea.close(); eb.close()


# ------------------------------------------------------------------------------------------------ 6. the zero model
def test_zero_delays_and_zero_bias_equal_the_model_switched_off():
    N = 5
    zero = (0, 0, np.zeros((N, NOBS), np.float32))
    (on,), (off,) = _rollout_pair(N, False, "elu", False, zero, modes=(True,)), _rollout_pair(N, False, "elu", False, None, modes=(True,))
    assert on["env"].sensor_model()["on"] and not off["env"].sensor_model()["on"]
    for name in ("observations", "actions", "actions_log_prob", "values", "rewards", "dones", "mu", "sigma"):
        assert torch.equal(getattr(on["st"], name), getattr(off["st"], name)), name
    assert torch.equal(on["obs"], off["obs"]) and torch.equal(on["lv"], off["lv"])
    _resets_inside(on["st"].dones.squeeze(-1).cpu().numpy() > 0)
    tape = _tape(N)
    recs = []
    for m in (zero, None):
        e, r = _start(N, m), torch.zeros((K, N, NOBS), device=DEV)
        e.step_tape(tape, record=dict(obs=r))
        recs.append(r)
        e.close()
    assert torch.equal(recs[0], recs[1])
    on["env"].close(); off["env"].close()


# ------------------------------------------------------------------------------------------------ 7. resets and state
def test_resets_clear_the_history_state_round_trips_and_off_is_off():
    N = 5
    tape, model = _tape(N), sn.model(N, 4)
    B, A = _start(N, model), _start(N)
    for t in range(3):
        B.step(tape[t]); A.step(tape[t])
    ring, count = B.sensor_state()
    assert (count == 3).all() and np.abs(ring[:, :3]).sum() > 0 and not ring[:, 3].any()
    B.reset_idx([1, 3]); A.reset_idx([1, 3])
    ring2, count2 = B.sensor_state()
    assert count2.tolist() == [3, 0, 3, 0, 3] and np.array_equal(ring2, ring)
    # the next reading of a reset env sees only itself, the others reach back
    y = A.step(tape[3])[0].cpu().numpy()
    got = B.step(tape[3])[0].cpu().numpy()
    for e in (1, 3):
        want = np.clip(y[e] + model[2][e], -CLIP, CLIP)
        want[sn.PASS] = y[e, sn.PASS]
        np.testing.assert_array_equal(got[e], want)
    assert not np.array_equal(got[2, sn.IMU], np.clip(y[2] + model[2][2], -CLIP, CLIP)[sn.IMU])      # env 2: d_imu = 2
    # set_sensor_state(sensor_state()) round-trips, as a tuple or as two arguments
    st = B.sensor_state()
    B.set_sensor_state(np.zeros_like(st[0]), np.zeros_like(st[1]))
    assert not B.sensor_state()[0].any() and not B.sensor_state()[1].any()
    B.set_sensor_state(st)
    np.testing.assert_array_equal(B.sensor_state()[0], st[0]); np.testing.assert_array_equal(B.sensor_state()[1], st[1])
    with pytest.raises(ValueError, match="set_sensor_state"):
        B.set_sensor_state(st[0][:, :3], st[1])
    m = B.sensor_model()
    assert m["on"] and np.array_equal(m["imu_delay"].cpu().numpy(), model[0]) and np.array_equal(m["joint_delay"].cpu().numpy(), model[1])
    assert np.array_equal(m["bias"].cpu().numpy(), model[2])
    # off: the next step is a model-less env's
    B.set_sensor_model(None, None, None)
    assert not B.sensor_model()["on"] and not B.sensor_model()["bias"].any()
    assert torch.equal(B.step(tape[4])[0], A.step(tape[4])[0]) and torch.equal(B.true_observations(), A.get_observations())
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------ 8. the draw on the device, the refusals
def test_device_draw_equals_the_host_function_and_bad_models_are_refused():
    from nightmare_rl_amd import _lib
    from test_sensor_host import KINDS, _draw
    N, off = 5, 7
    env = _start(N, offset=off)
    bmax = dict(lin_vel=0.2, ang_vel=0.05, gravity=0.02, dof_pos=0.03, dof_vel=0.4)
    m = env.draw_sensor_model((0, 3), (1, 2), bmax)
    assert m["on"] and not env.sensor_state()[1].any()
    for e in range(N):
        d, b = _draw(env._L, 11, off + e, (0, 1), (3, 2), [bmax[k] for k in KINDS])
        assert [int(m["imu_delay"][e]), int(m["joint_delay"][e])] == d.tolist(), e
        np.testing.assert_array_equal(m["bias"][e].cpu().numpy(), b)
    assert m["bias"].abs().sum() > 0 and not m["bias"][:, torch.from_numpy(sn.PASS).to(DEV)].any()
    env.step(torch.zeros((N, 18), device=DEV))
    before = env.sensor_model()
    cnt = env.sensor_state()[1].copy()
    bias = np.zeros((N, NOBS), np.float32)
    for kw, word in ((dict(imu_delay=[0, 1, 4, 0, 0]), "env 2 column 0"), (dict(joint_delay=[0, -1, 0, 0, 0]), "env 1 column 1"),
                     (dict(bias=np.where(np.arange(N * NOBS).reshape(N, NOBS) == 3 * NOBS + 20, np.nan, bias)), "env 3 column 20"),
                     (dict(bias=np.where(np.arange(N * NOBS).reshape(N, NOBS) == 4 * NOBS + 10, 0.5, bias)), "env 4 column 10")):
        with pytest.raises(_lib.NightmareHipError, match=word):
            env.set_sensor_model(**kw)
        after = env.sensor_model()
        assert after["on"] and all(torch.equal(after[k], before[k]) for k in ("imu_delay", "joint_delay", "bias"))
        np.testing.assert_array_equal(env.sensor_state()[1], cnt)           # the history was not cleared either
    with pytest.raises(ValueError, match="whole number"):
        env.set_sensor_model(imu_delay=0.5)
    with pytest.raises(ValueError, match="bias must be"):
        env.set_sensor_model(bias=np.zeros((N, 65), np.float32))
    with pytest.raises(_lib.NightmareHipError, match="above 3"):
        env.draw_sensor_model((0, 4), None, None)
    env.close()
