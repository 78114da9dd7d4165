"""Hidden-layer activations of the networks (rsl_rl v1.0.2 get_activation; reference envs/nightmare_v3_config.py:109 `activation = 'elu'
# can be elu, relu, selu, crelu, lrelu, tanh, sigmoid`) on the host side: the module, the name -> NM_ACT_* table, the C ABI's checks that
run before any device call. No GPU needed."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["elu", "selu", "relu", "crelu", "lrelu", "tanh", "sigmoid"]
REF_ACTOR, REF_CRITIC = [66, 54, 42, 30, 18], [66, 54, 42, 30, 1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from nightmare_rl_amd import _lib
    return _lib.load()


def _header_codes():
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bNM_ACT_([A-Z]+)\s*=\s*(\d+)", hdr)}
    n = int(re.search(r"#define\s+NM_NUM_ACTIVATIONS\s+(\d+)", hdr).group(1))
    return codes, n


@pytest.mark.parametrize("name", NAMES)
def test_actor_critic_constructs_for_every_reference_activation(name):
    from nightmare_rl_amd.rl import ActorCritic
    ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation=name)
    assert ac.activation_name == name
    acts = [m for m in list(ac.actor) + list(ac.critic) if not isinstance(m, nn.Linear)]
    assert len(acts) == 6
    if name == "crelu":         # rsl_rl v1.0.2's get_activation: "crelu" -> nn.ReLU()
        assert all(type(m) is nn.ReLU for m in acts)
    x = torch.randn(5, 66)
    assert ac.act_inference(x).shape == (5, 18) and ac.evaluate(x).shape == (5, 1)


def test_name_table_equals_the_header_enum():
    from nightmare_rl_amd import _lib
    codes, n = _header_codes()
    assert codes == {"elu": 0, "selu": 1, "relu": 2, "lrelu": 3, "tanh": 4, "sigmoid": 5} and n == 6
    assert set(_lib.ACTIVATIONS) == set(NAMES)
    for name, code in codes.items():
        assert _lib.ACTIVATIONS[name] == code
    assert _lib.ACTIVATIONS["crelu"] == codes["relu"]
    assert sorted(set(_lib.ACTIVATIONS.values())) == list(range(n))
    with pytest.raises(ValueError, match="gelu"):
        _lib.activation_code("gelu")


def test_library_exports_the_activation_entry_points(lib):
    from nightmare_rl_amd import _lib
    new = ["nm_policy_create_act", "nm_ppo_create_act", "nm_rollout_supported_act", "nm_rollout_ex", "nm_rollout_act_ex"]
    assert set(new) <= set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, s) for s in new)


def test_rollout_supported_act_for_every_code_and_no_other(lib):
    a = (ctypes.c_int32 * 5)(*REF_ACTOR)
    c = (ctypes.c_int32 * 5)(*REF_CRITIC)
    _, n = _header_codes()
    for code in range(n):
        assert lib.nm_rollout_supported_act(a, c, 4, code) == 1, code
    for code in (-1, n):
        assert lib.nm_rollout_supported_act(a, c, 4, code) == 0, code
    assert lib.nm_rollout_supported(a, c, 4) == 1                       # the ELU entry point as before
    other = (ctypes.c_int32 * 5)(66, 40, 24, 20, 18)
    assert lib.nm_rollout_supported_act(other, c, 4, 4) == 0            # not the compiled shape, whatever the activation


def test_unknown_activation_is_refused_before_any_device_call(lib):
    """Code 6 fails and the error names it - also on a machine without a GPU: the check precedes hipGetDeviceCount."""
    h = ctypes.c_void_p()
    dims = (ctypes.c_int32 * 4)(66, 64, 64, 18)
    assert lib.nm_policy_create_act(dims, 3, 6, 0, ctypes.byref(h)) != 0 and not h.value
    msg = lib.nm_last_error().decode()
    assert "activation" in msg and "6" in msg, msg
    a = (ctypes.c_int32 * 5)(*REF_ACTOR)
    c = (ctypes.c_int32 * 5)(*REF_CRITIC)
    assert lib.nm_ppo_create_act(a, c, 4, 6, 0, ctypes.byref(h)) != 0 and not h.value
    msg = lib.nm_last_error().decode()
    assert "activation" in msg and "6" in msg, msg
    assert lib.nm_ppo_create_act(a, c, 4, -1, 0, ctypes.byref(h)) != 0 and "-1" in lib.nm_last_error().decode()
    from nightmare_rl_amd.policy import PackedMLP
    with pytest.raises(ValueError, match="activation"):
        PackedMLP([66, 18], "cuda:0", activation="gelu")


def test_tanh_network_on_the_cpu_keeps_the_torch_path():
    from nightmare_rl_amd.rl import ActorCritic
    from nightmare_rl_amd.rl.fused import FusedCollector, FusedUpdate
    from nightmare_rl_amd.rl.ppo import PPO
    ac = ActorCritic(66, 66, 18, actor_hidden_dims=[54, 42, 30], critic_hidden_dims=[54, 42, 30], activation="tanh")
    assert not FusedCollector.supported(ac, "cpu") and not FusedUpdate.supported(ac, "cpu")
    ppo = PPO(ac, device="cpu")
    ppo.init_storage(8, 4, [66], [None], [18])
    assert ppo.fused is None and ppo.fused_update is None
    obs = torch.randn(8, 66)
    a = ppo.act(obs, obs)
    assert a.shape == (8, 18) and torch.isfinite(a).all()
