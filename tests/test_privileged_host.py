"""The privileged critic row, host side (no GPU): the column names, the numpy restatement of the row (envs/privileged.py) on hand-written
inputs, the library's export, and that nothing claims the hand-written kernels on a CPU device."""
import ctypes

import numpy as np
import torch

from nightmare_rl_amd import _lib
from nightmare_rl_amd.envs import privileged as P


def _defaults():
    # round numbers, not the model's: the table is checked, not the model
    return dict(mu=0.9, p_gain=20.0, kv=0.8, base_mass=2.0, base_ipos=np.array([0.01, 0.0, 0.02]), total_mass=3.0, grav=10.0, decimation=2)


def test_names():
    assert len(P.NAMES) == 23 == P.NUM_PRIVILEGED and len(set(P.NAMES)) == 23
    assert P.NUM_PRIVILEGED_OBS == 89 and P.NAMES[0] == "friction" and P.NAMES[-1] == "base_height"
    assert P.NAMES.index("gravity_x") == 8 and P.NAMES.index("wrench_force_x") == 16 and P.NAMES.index("latency_steps") == 7


def test_reference_on_hand_written_inputs():
    d = _defaults()
    obs = np.arange(2 * 66, dtype=np.float32).reshape(2, 66) / 7
    body = np.zeros((2, 20))
    body[:, 0:3] = [[0.02, 0.01, 0.02], [0.01, 0.0, 0.05]]
    body[:, 9] = [2.5, 1.5]
    row = P.privileged_reference(obs, d, base_height=[0.11, 0.12], mu=[0.5, 1.25], p_gain=[10.0, 30.0], kv=[0.4, 1.6], body_rows=body, latency=[0, 3],
                                 g=[[0.0, 0.0, -10.0], [5.0, 0.0, -5.0]], rate_limit=[np.inf, 0.25], d_gain=[0.0, 0.05],
                                 torque_limit=[[np.inf, np.inf, np.inf], [2.0, 4.0, 8.0]], force=[[30.0, 0.0, -15.0], [0.0, 0.0, 0.0]],
                                 torque=[[0.0, 3.0, 0.0], [0.0, 0.0, -6.0]])
    assert row.dtype == np.float32 and row.shape == (2, 89)
    assert np.array_equal(row[:, :66], obs)
    want = np.array([[0.5, 0.5, 0.5, 0.5, 0.01, 0.01, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.5, 0.0, 0.1, 0.0, 0.11],
                     [1.25, 1.5, 2.0, -0.5, 0.0, 0.0, 0.03, 1.5, 0.5, 0.0, -0.5, 4.0, 0.05, 0.5, 0.25, 0.125, 0.0, 0.0, 0.0, 0.0, 0.0, -0.2, 0.12]])
    np.testing.assert_allclose(row[:, 66:], want, rtol=1e-6, atol=1e-9)
    assert row[0, 66 + 11] == 0.0 and (row[0, 66 + 13:66 + 16] == 0.0).all()      # +inf -> exactly 0


def test_reference_defaults():
    d = _defaults()
    row = P.privileged_reference(np.zeros((3, 66)), d, base_height=0.2)
    want = np.zeros(23)
    want[[0, 1, 2, 10, 22]] = [0.9, 1.0, 1.0, -1.0, 0.2]
    assert np.array_equal(row[:, 66:], np.broadcast_to(want.astype(np.float32), (3, 23)))
    # the default ROWS (what the getters report while a kind is off) give the same values
    body = np.zeros((3, 20))
    body[:, 0:3], body[:, 9] = d["base_ipos"], d["base_mass"]
    row2 = P.privileged_reference(np.zeros((3, 66)), d, base_height=0.2, mu=d["mu"], p_gain=d["p_gain"], kv=d["kv"], body_rows=body, latency=0,
                                  g=[0.0, 0.0, -d["grav"]], rate_limit=np.inf, d_gain=0.0, torque_limit=np.inf, force=np.zeros(3), torque=np.zeros(3))
    assert np.array_equal(row, row2)


def test_model_defaults_are_rounded_to_the_envs_dtype():
    d32, d64 = P.model_defaults(20, 2, 1.0, 0.8, np.float32), P.model_defaults(20, 2, 1.0, 0.8, np.float64)
    assert d32["grav"] == float(np.float32(9.81)) and d64["grav"] == 9.81 and d32["decimation"] == 2
    assert d32["base_mass"] == float(np.float32(d64["base_mass"])) and 1.0 < d64["base_mass"] < d64["total_mass"]
    assert d32["base_ipos"].shape == (3,)


def test_switch_is_read_with_a_default():
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3Config
    assert not hasattr(NightmareV3Config().env, "privileged_obs") and not P.enabled(NightmareV3Config())

    class Cfg(NightmareV3Config):
        class env(NightmareV3Config.env):
            privileged_obs = True
    assert P.enabled(Cfg()) and Cfg().env.num_obs == 66


def test_library_exports_the_entry_points():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nm_privileged_obs", "nm_ppo_sample_prefix"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    hdr = open(_lib.HERE + "/../include/nightmare_hip.h").read()
    assert "int nm_privileged_obs(nm_env* env, const float* obs_dev, float* out_dev, void* stream);" in hdr
    assert "#define NM_NUM_PRIVILEGED 23" in hdr


def test_no_kernel_path_on_the_cpu_for_either_shape():
    from nightmare_rl_amd.rl import PPO, ActorCritic
    from nightmare_rl_amd.rl.fused import FusedCollector, FusedUpdate
    for n_critic in (66, 89):
        ac = ActorCritic(66, n_critic, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="elu")
        assert not FusedCollector.supported(ac, "cpu") and not FusedUpdate.supported(ac, "cpu")
    # and the torch path of an asymmetric PPO still works on the host, whatever the caller promises about the row
    torch.manual_seed(0)
    alg = PPO(ac, num_learning_epochs=1, num_mini_batches=2, device="cpu")
    alg.init_storage(4, 3, [66], [89], [18], critic_has_obs_prefix=True)
    assert alg.fused is None and alg.fused_update is None and alg.storage.privileged_observations.shape == (3, 4, 89)
    for _ in range(3):
        wide = torch.randn(4, 89)
        a = alg.act(wide[:, :66], wide)
        assert a.shape == (4, 18)
        alg.process_env_step(torch.randn(4), torch.zeros(4, dtype=torch.int64), {})
    alg.compute_returns(torch.randn(4, 89))
    vl, sl = alg.update()
    assert np.isfinite([vl, sl]).all()
