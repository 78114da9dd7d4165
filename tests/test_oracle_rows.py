"""The oracle's per-env rows (oracle/nm_oracle.h, nmo_rows) against the fp64 fixtures under tests/golden/ that the device paths are
checked against, and against themselves: CPU only.

  * rows set to their defaults change nothing, bit for bit;
  * every fixture with a zero payload is REPLAYED: from its recorded start state (state, buffers, action history, limited targets), under
    its recorded actions and command uniforms, 10 steps x 8 envs of the live oracle give the fixture's qpos, qvel, qw, obs, rew, done and
    ncon exactly. The sets that carry a payload need a library compiled against another model header and stay with their generators
    (tests/golden/make_*_goldens.py). No recorded key is left out: the step-start buffers dof_pos, dof_vel, act, cmd, ep_len, hist and
    lim are compared as well wherever the fixture holds them, and so are torque.npz's qfrc and margin.
    allrand.npz and allkinds.npz set 2 (payload 0) were NOT recorded against the committed nm_model_data.h: every set of these two files
    is compiled against emit_header(payload.modified_tables(dm, r)), dm = 0 included, and that derivation returns the base body's
    principal axes in another order and constants within an ulp of the committed ones (make_allrand_goldens.py asserts the two
    trajectories within 1e-12 of each other, not equal). Against oracle/libnm_oracle.so the replay of set 2 differs in 17 of the 200
    qpos words after the first step of `drop`, by at most 1.1e-16. It is therefore replayed, as exactly, on a library that
    oracle.build(header=...) compiles here against that header: the tables the set was recorded with;
  * per-env means per-env: a mixed batch equals uniform batches env for env, and two env objects in one process do not see each
    other's rows.
"""
import numpy as np
import pytest

from conftest import load_golden
import allkinds_tools
import allrand_tools

N, T = 8, 10
G0 = np.array([0.0, 0.0, -9.81])
STATE_KEYS = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len")


def set_rows(o, gravity=None, envp=None, delays=None, hist=None, servo=None, lim=None, torque=None, wrench=None):
    """gravity: the device's [.., 8] row (g, pad, gravity_vec, pad)."""
    gravity = None if gravity is None else np.broadcast_to(gravity, (o.N, 8))
    o.set_gravity(None if gravity is None else gravity[:, 0:3], None if gravity is None else gravity[:, 4:7])
    o.set_env_params(envp)
    o.set_action_latency(delays, hist)
    o.set_servo(servo, lim)
    o.set_torque_limit(torque)
    o.set_base_wrench(wrench)


def replay(orc, rec, lib_path=None, **rows):
    """rec: key -> [T or T + 1, 8, ...] of one recording."""
    o = orc.OracleEnv(N, seed=5, lib_path=lib_path)
    o.reset_idx()
    o.set_state(rec["qpos"][0], rec["qvel"][0], rec["qw"][0])
    o.set_buffers(dof_pos=rec["dof_pos"][0], dof_vel=rec["dof_vel"][0], actions=rec["act"][0], commands=rec["cmd"][0], ep_len=rec["ep_len"][0])
    set_rows(o, hist=rec["hist"][0] if "hist" in rec else None, lim=rec["lim"][0] if "lim" in rec else None, **rows)
    for t in range(T):
        obs, _, done, _ = o.step(rec["actions"][t], cmd_u=rec["cmd_u"][t].astype(np.float64))
        q, v, w = o.get_state()
        b = o.get_buffers()
        got = dict(qpos=q, qvel=v, qw=w, dof_pos=b["dof_pos"], dof_vel=b["dof_vel"], act=b["actions"], cmd=b["commands"], ep_len=b["ep_len"])
        for key in STATE_KEYS:
            np.testing.assert_array_equal(got[key], rec[key][t + 1], err_msg=f"{key} after step {t}")
        np.testing.assert_array_equal(obs, rec["obs"][t], err_msg=f"obs of step {t}")
        np.testing.assert_array_equal(o.rew64, rec["rew"][t], err_msg=f"rew of step {t}")
        np.testing.assert_array_equal(done.astype(np.uint8), rec["done"][t], err_msg=f"done of step {t}")
        np.testing.assert_array_equal([o.data(i).ncon for i in range(N)], rec["ncon"][t], err_msg=f"ncon of step {t}")
        if "hist" in rec:
            np.testing.assert_array_equal(o.action_history()[0], rec["hist"][t + 1], err_msg=f"hist after step {t}")
        if "lim" in rec:
            np.testing.assert_array_equal(o.servo_state()[1], rec["lim"][t + 1], err_msg=f"lim after step {t}")
        if "qfrc" in rec:
            np.testing.assert_array_equal([o.data(i).np("qfrc_actuator")[6:] for i in range(N)], rec["qfrc"][t], err_msg=f"qfrc of step {t}")
            np.testing.assert_array_equal(o.torque_limit()[1].min(), rec["margin"][t], err_msg=f"margin of step {t}")


def recording(g, pop, k=None, prefix=""):
    head = f"{prefix}{pop}_"
    return {key[len(head):]: (v if k is None else v[k]) for key, v in g.items() if key.startswith(head)}


def test_replay_env_params(oracle_mod):
    g = dict(load_golden("env_params.npz"))
    for k, row in enumerate(g["sets"]):
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), envp=row)


def test_replay_gravity(oracle_mod):
    g = dict(load_golden("gravity.npz"))
    for k, row in enumerate(g["rows"]):
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), gravity=row)


def test_replay_latency(oracle_mod):
    g = dict(load_golden("latency.npz"))
    for pop in ("drop", "stand"):
        replay(oracle_mod, recording(g, pop), delays=g["delays"])


def test_replay_servo(oracle_mod):
    g = dict(load_golden("servo.npz"))
    rows = np.stack([g["rate"], g["d_gain"]], axis=1)
    for rec, delays in (("S", None), ("SL", g["delays"])):
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, prefix=rec + "_"), delays=delays, servo=rows)


def test_replay_torque(oracle_mod):
    g = dict(load_golden("torque.npz"))
    for k, fmax in enumerate(g["sets"]):
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), torque=fmax, envp=[1.0, 20.0, g["kv"][k]])


def test_replay_wrench(oracle_mod):
    g = dict(load_golden("wrench.npz"))
    zero_payload = [k for k in range(len(g["sets"])) if not g["payload"][k].any()]
    assert zero_payload == [0, 1, 2, 4]
    for k in zero_payload:
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), wrench=g["sets"][k])


@pytest.fixture(scope="module")
def payload0_lib(oracle_mod, tmp_path_factory):
    """The library of the payload sets' own recipe at dm = 0 (see the module docstring)."""
    from nightmare_rl_amd.model import compile_model, payload
    d = tmp_path_factory.mktemp("payload0")
    compile_model.emit_header(payload.modified_tables(0.0, np.zeros(3)), str(d / "nm_model_data.h"))
    return oracle_mod.build(header=str(d / "nm_model_data.h"), out=str(d / "libnm_oracle_payload0.so"))


def test_replay_allrand(oracle_mod, payload0_lib):
    g = allrand_tools.load()
    zero_payload = [k for k in range(4) if not g["payloads"][k].any()]
    assert zero_payload == [2]
    for k in zero_payload:
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), payload0_lib, gravity=g["grav_rows"][k], envp=g["envp_rows"][k], delays=g["delays"])


def test_replay_allkinds(oracle_mod, payload0_lib):
    g = allkinds_tools.load()
    zero_payload = [k for k in range(4) if not g["payloads"][k].any()]
    assert zero_payload == [2]
    for k in zero_payload:
        for pop in ("drop", "stand"):
            replay(oracle_mod, recording(g, pop, k), payload0_lib, gravity=g["grav_rows"][k], envp=g["envp_rows"][k], delays=g["delays"],
                   servo=g["servo_rows"], torque=g["torque_rows"][k], wrench=g["wrench_rows"][k])


def run(o, steps, seed=5):
    """`drop`: random actions from the initial pose. Returns every step's state, obs, rew, done."""
    rng = np.random.default_rng(seed)
    o.reset_idx()
    out = []
    for _ in range(steps):
        a = rng.uniform(-1, 1, (o.N, 18)).astype(np.float32)
        cu = rng.uniform(0, 1, (o.N, 4)).astype(np.float32).astype(np.float64)
        obs, _, done, _ = o.step(a, cmd_u=cu)
        out.append(np.concatenate([np.concatenate(o.get_state(), axis=1), o.obs64, o.rew64[:, None], done[:, None]], axis=1))
    return np.stack(out)


@pytest.mark.parametrize("num_threads", [1, 4])
def test_default_rows_change_nothing(oracle_mod, num_threads):
    never = run(oracle_mod.OracleEnv(N, seed=5, num_threads=num_threads), 17)
    o = oracle_mod.OracleEnv(N, seed=5, num_threads=num_threads)
    set_rows(o, gravity=np.concatenate([G0, [0.0], G0, [0.0]]), envp=[1.0, 20.0, 0.8], delays=np.zeros(N, np.int32),
             hist=np.zeros((N, 3, 18), np.float32), servo=[np.inf, 0.0], lim=np.tile([0.0, -np.pi / 5, 0.0], (N, 6)), torque=[np.inf] * 3,
             wrench=np.zeros(6))
    np.testing.assert_array_equal(run(o, 17), never)


def torque_wrench_rows(o, sets):
    tq, wr = load_golden("torque.npz"), load_golden("wrench.npz")
    o.set_torque_limit(tq["sets"][sets])
    o.set_env_params(np.stack([np.ones(len(sets)), np.full(len(sets), 20.0), tq["kv"][sets]], axis=1))
    o.set_base_wrench(wr["sets"][sets])
    return o


def test_mixed_batch_equals_uniform_batches(oracle_mod):
    n = 10
    mixed = run(torque_wrench_rows(oracle_mod.OracleEnv(n, seed=5, num_threads=4), np.arange(n) % 5), 10)
    uniform = [run(torque_wrench_rows(oracle_mod.OracleEnv(n, seed=5), np.full(n, k)), 10) for k in range(5)]
    for e in range(n):
        np.testing.assert_array_equal(mixed[:, e], uniform[e % 5][:, e], err_msg=f"env {e}")
    assert np.abs(uniform[1][:, 0] - uniform[0][:, 0]).max() > 1e-5      # the rows do act


def test_two_envs_in_one_process(oracle_mod):
    """Stepped alternately, each equals its solo run: no row lives outside its env object."""
    def make(k):
        return torque_wrench_rows(oracle_mod.OracleEnv(N, seed=5, num_threads=2), np.full(N, k))

    solo = [run(make(k), 10) for k in (3, 4)]
    a, b = make(3), make(4)
    rng = [np.random.default_rng(5), np.random.default_rng(5)]
    got = [[], []]
    a.reset_idx(); b.reset_idx()
    for _ in range(10):
        for i, o in enumerate((a, b)):
            act = rng[i].uniform(-1, 1, (N, 18)).astype(np.float32)
            cu = rng[i].uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            _, _, done, _ = o.step(act, cmd_u=cu)
            got[i].append(np.concatenate([np.concatenate(o.get_state(), axis=1), o.obs64, o.rew64[:, None], done[:, None]], axis=1))
    for i in range(2):
        np.testing.assert_array_equal(np.stack(got[i]), solo[i])
    assert np.abs(solo[0] - solo[1]).max() > 1e-5
