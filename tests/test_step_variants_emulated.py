"""The step's lean configuration traits (nm::CfgLean: what nm_step_lean.hip compiles the step kernel with) against the generic ones
(nm::CfgAsk), both as host SIMT emulations of the device source from one library (tests/emul/nm_emul.cpp): over the goldens
recorded with the default configuration the two must agree BIT FOR BIT in everything a step returns and leaves behind, and the lean
one must refuse what the host refuses to launch the lean kernel for."""
import numpy as np
import pytest

from conftest import load_golden

DEFAULT_CONFIG = ["env_reset_rollout.npz", "env_timeouts.npz", "env_falls.npz", "env_manycontacts.npz"]
KEPT = ("qpos", "qvel", "qwarm", "dofpos", "dofvel", "act", "cmd", "epsum")


@pytest.fixture(scope="module")
def lean():
    from emul import emul as em
    em.build(em.BASE)
    return em


@pytest.mark.parametrize("name", DEFAULT_CONFIG)
def test_lean_traits_equal_generic_traits_over_the_default_config_goldens(lean, name):
    """Teacher-forced on the golden's states (falls, time-outs, more than 16 contacts), commands from the counter RNG on both sides
    (injected uniforms are an input the lean kernel does not take)."""
    g = load_golden(name)
    from test_oracle_env_golden import golden_config
    T, N = g["actions"].shape[:2]
    envs = [lean.EmulEnv(N, lean=True), lean.EmulEnv(N, lean=False)]
    for e in envs:
        e.configure(**golden_config(g))         # the golden's own record of the default configuration: the lean env refuses any other
    qpos, qvel, qw = g["init_qpos"], g["init_qvel"], g["init_qacc_warmstart"]
    dofpos, dofvel, cmd, ep = g["init_dof_pos"], g["init_dof_vel"], g["init_commands"], g["init_ep_len"]
    act = np.zeros((N, 18))
    n_done = n_to = 0
    for t in range(T):
        out = []
        for e in envs:
            e.set("qpos", qpos); e.set("qvel", qvel); e.set("qwarm", qw); e.set("dofpos", dofpos); e.set("dofvel", dofvel)
            e.set("cmd", cmd); e.set("act", act)
            e.eplen[:] = ep
            res = e.step(g["actions"][t])
            out.append(res + tuple(e.get(k) for k in KEPT) + (np.array(e.eplen), e.hull_cache(), e.stat_sum, e.stat_cnt) + e.get_feet_state())
        for k, (a, b) in enumerate(zip(*out)):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} step {t} item {k}")
        n_done += int(out[0][2].sum()); n_to += int(out[0][3].sum())
        qpos, qvel, qw = g["qpos"][t], g["qvel"][t], g["qacc_warmstart"][t]
        dofpos, dofvel, cmd, ep = g["dof_pos"][t], g["dof_vel"][t], g["commands"][t], g["ep_len"][t]
        act = np.clip(g["actions"][t].astype(np.float32) * np.float32(0.2), -1, 1).astype(np.float64)
    assert envs[0].refused() == 0
    if name in ("env_falls.npz", "env_timeouts.npz"):
        assert n_done >= 1
    if name == "env_timeouts.npz":
        assert n_to >= 1


def test_lean_emulation_refuses_what_the_lean_kernel_is_not_launched_for(lean):
    N = 2
    a = np.zeros((N, 18), np.float32)
    e = lean.EmulEnv(N, lean=True)
    e.step(a)
    assert e.refused() == 0
    e.step(a, cmd_u=np.full((N, 4), 0.5))
    assert e.refused() == 1
    e.step(a, physics_only=True)
    assert e.refused() == 2
    e.step(a, want_dbg=True)
    assert e.refused() == 3
    e.configure({"termination": -200.0, "ang_vel_xy": -0.05})
    e.step(a)
    assert e.refused() == 4
    e.configure({"termination": -200.0}, tibia_contact_mode=2)
    e.step(a)
    assert e.refused() == 5
    e.configure({"termination": -200.0})
    e.step(a)
    assert e.refused() == 5
