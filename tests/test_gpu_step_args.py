"""k_env_step reads its launch arguments from the kernarg segment (scalar loads, scalar-base global accesses) while the K-step tape kernel
keeps the copy in LDS and the 64-bit address form: the two must stay equal BIT FOR BIT, for every per-env row level (each is an
instantiation of its own), at env counts that leave a half-empty last wave (1, 63) and that cross a ticket group (130). The only
tolerance is the project's for extras['episode'], a sum through float atomics (atol 1e-6, rtol 1e-4, as in test_gpu_tape.py)."""
import numpy as np
import pytest
import torch

from test_gpu_play import _env
from test_gpu_tape import _assert_same_env, _records, _tape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 40            # > 32 steps = one episode of 0.5 s: every env times out inside the run, falls and command resamples come with the random actions
LEVELS = ["none", "gains", "payload", "latency"]


def _switch_on(env, level):
    """Each level of per-env rows the host can switch on (nm_env_rows.h): the step kernel's EP = 0 ... 3."""
    if level in ("gains", "latency"):
        env.draw_env_params(friction_range=(0.6, 1.2), stiffness_multiplier_range=(0.8, 1.2), damping_multiplier_range=(0.8, 1.2))
    if level in ("payload", "latency"):
        env.draw_base_payload(mass_range=(0.0, 1.0), com_range=(-0.03, 0.03))
    if level == "latency":
        env.draw_action_latency(0, 3)


def _pair(N, level, ep_s=0.5):
    envs = [_env(N, episode_length_s=ep_s) for _ in range(2)]
    for e in envs:
        e.reset()
        _switch_on(e, level)
    return envs


# ------------------------------------------------------------------------------------------------ 1. step() x T vs the tape kernel
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("N", [1, 2, 63, 130])
def test_step_equals_the_tape_kernel_bit_for_bit(N, level):
    """T x step(actions[t]) against step_tape(actions) from the same start: what every step returned (observation, reward, reset flag),
    extras['time_outs'], the final buffers, episode lengths, state (qpos / qvel / warm start), kept buffers incl. the episode sums, feet
    state, counters - exactly."""
    ea, eb = _pair(N, level)
    actions = _tape(T, N)
    rec = _records(T, N)
    ob = eb.step_tape(actions, record=rec)
    n_to = torch.zeros(N, device=DEV)
    for t in range(T):
        oa, _, rew, done, extras = ea.step(actions[t])
        assert torch.equal(oa, rec["obs"][t]) and torch.equal(rew, rec["rew"][t]) and torch.equal(done.to(torch.uint8), rec["done"][t]), t
        if bool((done > 0).any()):
            n_to += extras["time_outs"] * (done > 0).float()
    assert float(n_to.min()) >= 1, "every env must time out within the run"
    _assert_same_env(ea, eb, oa, ob)
    assert torch.equal(ea.extras["time_outs"], eb.extras["time_outs"])
    torch.testing.assert_close(ea._ep_stats, eb._ep_stats, atol=1e-6, rtol=1e-4)
    if level == "latency":
        assert torch.equal(ea.action_history(), eb.action_history())
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 2. pointers are read anew by every launch
def test_two_captured_steps_replayed_read_their_own_observation_pointer():
    """Two consecutive step() calls captured into one graph and replayed three times against six eager steps. The observation buffers
    alternate, so the two launches' arguments differ in `obs` (and in `actions`): a pointer kept from the other launch fails here."""
    N = 63
    ea, eb = _pair(N, "none")
    acts = _tape(2, N)
    for e in (ea, eb):
        e.step(acts[0])                       # extras exist, both observation buffers have been handed out once
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o0 = ea.step(acts[0])[0]
        o1 = ea.step(acts[1])[0]
    assert o0.data_ptr() != o1.data_ptr()
    for r in range(3):
        g.replay()
        p0 = eb.step(acts[0])[0].clone()
        p1 = eb.step(acts[1])[0].clone()
        torch.cuda.synchronize()
        assert torch.equal(o0, p0) and torch.equal(o1, p1), r
        assert torch.equal(ea.rew_buf, eb.rew_buf) and torch.equal(ea.reset_buf, eb.reset_buf) and torch.equal(ea.time_out_buf, eb.time_out_buf), r
    for x, y in zip(ea.get_state(), eb.get_state()):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(ea.episode_length_buf, eb.episode_length_buf)
    del g
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------------------------------------ 3. the closing wave's other arguments
def test_replaced_time_outs_tensor_is_rewritten_in_full_like_the_tape_kernel_does():
    """A time-out tensor the last refresh did not write (here filled with 7) comes out completely rewritten: step() - its closing wave
    reads `time_outs`, `to_owner`, `N` from the kernarg segment - against a one-row tape on a second env, and against the known answer."""
    N = 63
    ea, eb = _pair(N, "none", ep_s=None)
    ids = torch.tensor([0, 31, 62])
    a = torch.zeros(1, N, 18, device=DEV)
    for e in (ea, eb):
        e.step(a[0])
        e.time_out_buf = torch.full((N,), 7.0, device=DEV)
        e.extras.pop("time_outs", None); e._fill_extras()
        e.episode_length_buf = torch.zeros(N, dtype=torch.int64, device=DEV)
        e.episode_length_buf[ids] = int(e.max_episode_length)         # + 1 > max_episode_length: these time out in this step
    ea.step(a[0])
    eb.step_tape(a)
    want = torch.zeros(N, device=DEV); want[ids] = 1
    assert torch.equal(ea.extras["time_outs"], want) and torch.equal(eb.extras["time_outs"], want)
    assert torch.equal(ea.reset_buf, eb.reset_buf) and torch.equal(ea.obs_buf, eb.obs_buf)
    for e in (ea, eb):
        e.close()


@pytest.mark.parametrize("level", ["none", "gains"])
def test_step_physics_moves_the_state_as_a_full_step_without_resets_does(level):
    """step_physics (the same kernel with physics_only set: no epilogue, servo command from qpos itself) against step() on a second env
    whose dof_pos buffer holds qpos[7:]: while no env resets, both leave the same qpos / qvel / warm start, bit for bit."""
    N = 63
    ea, eb = _pair(N, level, ep_s=None)
    a = _tape(3, N)
    for e in (ea, eb):
        qpos, _, _ = e.get_state()
        e.set_buffers(dof_pos=qpos[:, 7:])
    for t in range(3):
        ea.step_physics(a[t])
        done = eb.step(a[t])[3]
        assert int(done.sum()) == 0, "the comparison needs steps without a reset"
        for x, y in zip(ea.get_state(), eb.get_state()):
            np.testing.assert_array_equal(x, y)
    for e in (ea, eb):
        e.close()
