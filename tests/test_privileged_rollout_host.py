"""The one-launch rollout with privileged critic observations, host side (no GPU): the three entry points are declared and exported,
nm_rollout_supported_priv accepts the 66 / 89 networks and nothing else, the ctypes mirror of nm_rollout_priv_args, and the runner's
switch is off unless asked for."""
import ctypes as C
import os
import re

import pytest

from nightmare_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nm_rollout_supported_priv", "nm_rollout_priv", "nm_rollout_act_priv")


def test_the_three_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    declared = set(re.findall(r"\b(nm_[a-z_0-9]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTS, s
    assert "nm_rollout_priv_args" in hdr
    # each new declaration cites the reference lines it stands for, as its neighbours do
    for s in NEW:
        at = hdr.index(s + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert re.search(r"(train\.py|nightmare_v3_config\.py):\d+", comment), (s, comment)


ACT_ELU, ACT_TANH = _lib.ACTIVATIONS["elu"], _lib.ACTIVATIONS["tanh"]
CASES = [  # actor dims, critic dims, layers, activation, privileged answer, symmetric answer
    ((66, 54, 42, 30, 18), (89, 54, 42, 30, 1), 4, ACT_ELU, 1, 0),
    ((66, 54, 42, 30, 18), (89, 54, 42, 30, 1), 4, ACT_TANH, 1, 0),
    ((66, 54, 42, 30, 18), (66, 54, 42, 30, 1), 4, ACT_ELU, 0, 1),
    ((89, 54, 42, 30, 18), (66, 54, 42, 30, 1), 4, ACT_ELU, 0, 0),
    ((66, 54, 42, 30, 18), (90, 54, 42, 30, 1), 4, ACT_ELU, 0, 0),
    ((66, 54, 42, 18), (89, 54, 42, 1), 3, ACT_ELU, 0, 0),
    ((66, 256, 256, 30, 18), (89, 256, 256, 30, 1), 4, ACT_ELU, 0, 0),
    ((66, 54, 42, 30, 18), (89, 54, 42, 30, 1), 4, 99, 0, 0),
    ((66, 54, 42, 30, 18), (66, 54, 42, 30, 1), 4, 99, 0, 0),
]


@pytest.mark.parametrize("a,c,n,act,priv,sym", CASES)
def test_supported_priv_answers(a, c, n, act, priv, sym):
    L = _lib.load()
    ad, cd = (C.c_int32 * len(a))(*a), (C.c_int32 * len(c))(*c)
    assert L.nm_rollout_supported_priv(ad, cd, n, act) == priv
    assert L.nm_rollout_supported_act(ad, cd, n, act) == sym      # unchanged: the symmetric question keeps its answers
    assert L.nm_rollout_supported_priv(None, cd, n, act) == 0 and L.nm_rollout_supported_priv(ad, None, n, act) == 0


def test_every_known_activation_is_supported():
    L = _lib.load()
    ad, cd = (C.c_int32 * 5)(66, 54, 42, 30, 18), (C.c_int32 * 5)(89, 54, 42, 30, 1)
    for name, code in _lib.ACTIVATIONS.items():
        assert L.nm_rollout_supported_priv(ad, cd, 4, code) == 1, name


def test_struct_mirror_is_three_pointers():
    assert C.sizeof(_lib.NmRolloutPrivArgs) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in _lib.NmRolloutPrivArgs._fields_] == ["priv0_dev", "priv_final_dev", "s_priv"]
    hdr = open(os.path.join(ROOT, "include", "nightmare_hip.h")).read()
    body = hdr[hdr.rindex("typedef struct", 0, hdr.index("} nm_rollout_priv_args")):hdr.index("} nm_rollout_priv_args")]
    assert re.findall(r"\b(priv0_dev|priv_final_dev|s_priv)\s*;", body) == ["priv0_dev", "priv_final_dev", "s_priv"]


def test_null_env_is_refused_by_both_launching_entry_points():
    L = _lib.load()
    assert L.nm_rollout_priv(None, None, None, ACT_ELU, None) != 0
    assert L.nm_rollout_act_priv(None, None, None, 0, None, 0, None, None, None, None, None, None, None, ACT_ELU, None) != 0


def test_runner_switch_defaults_to_off():
    from nightmare_rl_amd.envs.helpers import class_to_dict
    from nightmare_rl_amd.envs.nightmare_v3_config import NightmareV3ConfigPPO
    from nightmare_rl_amd.rl import runner
    assert runner.PRIVILEGED_ROLLOUT_DEFAULT is False
    assert "privileged_rollout" not in class_to_dict(NightmareV3ConfigPPO())["runner"]      # the reference's config tree is unchanged
    src = open(os.path.join(ROOT, "train.py")).read()
    assert "--privileged-rollout" in src and re.search(r'"--privileged-rollout", action="store_true", default=False', src)
