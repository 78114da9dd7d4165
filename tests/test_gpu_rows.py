"""The four kinds of per-env rows together on the device - friction / gains, body rows (base payload), actuation latency, gravity vectors:
the walk of tests/rows_walk.py over every single-kind on / off transition from every state of the other three kinds, through NightmareV3Env. After every
toggle the env that took the walk must be indistinguishable from a fresh env of the same seed put directly into that state: the same
reported rows (the values set for the kinds that are on, what a never-touched env reports for the kinds that are off), and a step and a
physics-only step from the same start that agree bit for bit. N = 3 in fp32 (one full wave and a half-empty one), N = 2 in fp64 (one env
per wave). Exact comparisons; 65 small envs and 256 steps per dtype."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from rows_walk import WALK, Walk
from test_gpu_latency import ENVP_SETS, PAYLOADS
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, T0 = 5, 2      # T0: the fixture step the start state is taken from (its action history is not zero any more)


@pytest.fixture(scope="module")
def G():
    return load_golden("latency.npz")


def toggle(env, kind, values):
    """Set `kind` to values[kind], or switch it off where there is none."""
    if kind == "F":
        f = values.get("F")
        env.set_env_params(*(() if f is None else (f[:, 0], f[:, 1], f[:, 2])))
    elif kind == "B":
        b = values.get("B")
        env.set_base_payload(*(() if b is None else (b[:, 0], b[:, 1:])))
    elif kind == "L":
        env.set_action_latency(values.get("L"))
    else:
        g = values.get("G")
        env.set_gravity(*((None,) if g is None else (g[:, 0:3], g[:, 4:7])))


def reported(env):
    torch.cuda.synchronize()
    p, g = env.env_params(), env.gravity()
    return (torch.stack([p["mu"], p["p_gain"], p["kv"]], dim=1).cpu().numpy(), env.base_payload()["rows"].cpu().numpy(),
            env.action_latency().cpu().numpy(), torch.cat([g["g"], g["gravity_vec"]], dim=1).cpu().numpy())


def two_steps(env, g):
    """From the dropped population's state of step T0 (state, buffers, feet state, command uniforms, action history): step(a), then
    step_physics(a); everything they leave behind."""
    n = env.num_envs
    pick = lambda k: g[f"drop_{k}"][T0, :n]
    env.set_state(pick("qpos"), pick("qvel"), pick("qw"))
    env.set_buffers(dof_pos=pick("dof_pos"), dof_vel=pick("dof_vel"), actions=pick("act"), commands=pick("cmd"), episode_sums=np.zeros((n, 16)))
    env.set_feet_state(np.zeros((n, 6)), np.zeros((n, 6), np.uint8), np.zeros((n, 6), np.uint8))
    env.episode_length_buf = torch.from_numpy(np.asarray(pick("ep_len"), np.int64)).to(DEV)
    env.set_command_uniforms(pick("cmd_u").astype(np.float64))
    env.set_action_history(pick("hist"))
    a = torch.from_numpy(pick("actions")).to(DEV)
    obs, _, rew, done, extras = env.step(a)
    out = [obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy(), extras["time_outs"].cpu().numpy().copy()]
    env.step_physics(a)
    torch.cuda.synchronize()
    b = env.get_buffers()
    return out + list(env.get_state()) + [b[k] for k in sorted(b)] + [env.action_history().cpu().numpy()]


@pytest.mark.parametrize("N,dtype", [(3, torch.float32), (2, torch.float64)], ids=["fp32", "fp64"])
def test_an_env_that_took_the_walk_equals_a_fresh_env_put_into_that_state(G, N, dtype):
    from nightmare_rl_amd.model import payload
    real = np.float64 if dtype == torch.float64 else np.float32
    walker = make_env(N, dtype=dtype, seed=SEED)
    dflt = reported(walker)      # what a never-touched env reports: the model's own rows, zero delays
    assert not dflt[2].any()
    walk = Walk(N, ENVP_SETS, PAYLOADS, load_golden("gravity.npz")["rows"])
    before, steps_that_differed = None, 0
    for i, kind, on in walk:
        toggle(walker, kind, walk.values)
        fresh = make_env(N, dtype=dtype, seed=SEED)
        for k in walk.values:
            toggle(fresh, k, walk.values)
        # (a) the reported rows: walker = fresh = what was set for the kinds that are on, the never-touched env's for the kinds that are off
        want = list(dflt)
        if "F" in walk.values:
            want[0] = walk.values["F"].astype(real)
        if "B" in walk.values:
            want[1] = payload.payload_rows(walk.values["B"][:, 0], walk.values["B"][:, 1:]).astype(real)
        if "L" in walk.values:
            want[2] = walk.values["L"]
        if "G" in walk.values:
            want[3] = walk.values["G"][:, [0, 1, 2, 4, 5, 6]].astype(real)
        for w, x, y in zip(want, reported(walker), reported(fresh)):
            np.testing.assert_array_equal(x, y, err_msg=f"toggle {i} ({kind}): walker against fresh")
            np.testing.assert_array_equal(x, w, err_msg=f"toggle {i} ({kind}): walker against what was set")
        # (b) one step and one physics-only step from the same start: bit-identical
        ow, of = two_steps(walker, G), two_steps(fresh, G)
        for k, (x, y) in enumerate(zip(ow, of)):
            np.testing.assert_array_equal(x, y, err_msg=f"toggle {i} ({kind}), output {k}")
        if before is not None:
            steps_that_differed += any((x != y).any() for x, y in zip(ow, before))
        before = ow
        fresh.close()
    for x, y in zip(reported(walker), dflt):      # the walk ends all-off
        np.testing.assert_array_equal(x, y)
    # the toggles are not no-ops: each changes at least one env's servo gains, base inertia, delay or gravity, which two steps of a moving robot show
    assert steps_that_differed == len(WALK) - 1
    walker.close()
