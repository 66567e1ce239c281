"""The policy randomisation (tsidb_policy_randomize / _perturb / _reset_noise, PolicyRandomization), the parts that need no
GPU: the binding against the header, both libraries' exports, the launches a randomised PolicyEnv.step() makes, and the
configurations the host rejects."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_host import bare_env  # noqa: E402

NAMES = ("tsidb_policy_randomize", "tsidb_policy_perturb", "tsidb_policy_reset_noise")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text, en = HEADER, header_enums("TSIDB_POL_DR_")
    assert len(en) == len(_lib.POL_DR_FIELDS) + 1
    for k in _lib.POL_DR_FIELDS:
        assert getattr(_lib, "POL_DR_" + k.upper()) == en["TSIDB_POL_DR_" + k.upper()], k
    assert _lib.POL_DR_NPARAMS == en["TSIDB_POL_DR_NPARAMS"] == 23
    # the two base velocity amplitudes take three slots, every other field one, nothing overlaps
    starts = [en["TSIDB_POL_DR_" + k.upper()] for k in _lib.POL_DR_FIELDS] + [en["TSIDB_POL_DR_NPARAMS"]]
    width = {k: b - a for k, a, b in zip(_lib.POL_DR_FIELDS, starts, starts[1:])}
    assert width == {k: 3 if k in ("reset_base_lin_vel", "reset_base_ang_vel") else 1 for k in _lib.POL_DR_FIELDS}
    # the key layout is in the header
    assert "key = seed + ((stream * 256 + column) * 2^32)" in text
    # prototypes and exports of both libraries
    assert_prototypes(NAMES)


def test_randomization_is_exported_and_defaults_to_off():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv, PolicyRandomization
    assert tsid_control_amd.PolicyRandomization is PolicyRandomization
    assert [f.name for f in __import__("dataclasses").fields(PolicyRandomization)] == list(_lib.POL_DR_FIELDS)
    p = PolicyRandomization().params(default_seed=5)
    assert p.shape == (_lib.POL_DR_NPARAMS,) and p[_lib.POL_DR_SEED] == 5 and not p[1:].any()
    assert PolicyEnv.randomization is None and PolicyEnv._dr_push is False and PolicyEnv._dr_reset is False
    p = PolicyRandomization.of(dict(seed=2, reset_base_lin_vel=(0.1, 0.2, 0.3), reset_base_ang_vel=0.5, push_interval=7, push_duration=2)).params()
    assert list(p[_lib.POL_DR_RESET_BASE_LIN_VEL:_lib.POL_DR_RESET_BASE_LIN_VEL + 3]) == [0.1, 0.2, 0.3]
    assert list(p[_lib.POL_DR_RESET_BASE_ANG_VEL:_lib.POL_DR_RESET_BASE_ANG_VEL + 3]) == [0.5] * 3
    assert p[_lib.POL_DR_SEED] == 2 and p[_lib.POL_DR_PUSH_INTERVAL] == 7 and p[_lib.POL_DR_PUSH_DURATION] == 2


@pytest.mark.parametrize("bad,msg", [
    (dict(reset_joint_pos=float("nan")), "non-finite"), (dict(noise_gravity=float("inf")), "non-finite"),
    (dict(reset_joint_vel=-0.1), "negative"), (dict(noise_joint_pos=-1e-9), "negative"), (dict(reset_lift=-0.01), "negative"),
    (dict(push_interval=-1), "negative"), (dict(command_interval=-3), "negative"), (dict(reset_base_lin_vel=(0.1, -0.1, 0.0)), "negative"),
    (dict(push_interval=3, push_duration=4), "push_duration > push_interval"),
    (dict(push_interval=5, push_duration=1, push_force_lo=2.0, push_force_hi=1.0), "push_force_lo > push_force_hi"),
    (dict(command_zero_prob=1.5), r"\[0, 1\]"), (dict(command_zero_prob=-0.5), "negative"),
    (dict(seed=2 ** 32), "seed"), (dict(env_offset=0.5), "env_offset"), (dict(push_interval=2.5, push_duration=1), "push_interval"),
    (dict(reset_base_ang_vel=(1.0, 2.0)), "reset_base_ang_vel"), (dict(reset_yaw="wide"), "reset_yaw"),
    (dict(reset_jiont_pos=0.1), "unknown randomization fields"),
])
def test_rejected_configurations_raise_with_a_message(bad, msg):
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyRandomization
    with pytest.raises(_lib.TsidbError, match=msg):
        PolicyRandomization.of(bad).params()
    with pytest.raises(_lib.TsidbError, match="PolicyRandomization or a dict"):
        PolicyRandomization.of([1, 2, 3])


def test_randomised_step_is_act_perturb_sim_reward_reset_noise_obs():
    from tsid_control_amd import _lib
    for push, noise in ((True, True), (True, False), (False, True)):
        env, calls = bare_env(decimation=10)
        wc = env.wc
        wc.NB, wc.xfrc = 3, torch.zeros(3, 3, 6, dtype=torch.float64)
        env._dr_push, env._dr_reset = push, noise
        action = torch.zeros(3, wc.NA, dtype=torch.float64)
        obs, reward, done, info = env.step(action)
        names = [c[0] for c in calls]
        assert names == ["tsidb_policy_act"] + ["tsidb_policy_perturb"] * push + ["tsidb_sim_ctrl"] * 2 + ["tsidb_policy_reward", "tsidb_reset_done"] + \
            ["tsidb_policy_reset_noise"] * noise + ["tsidb_policy_obs"]
        by = {c[0]: c[1] for c in calls}
        if push:
            assert len(by["tsidb_policy_perturb"]) == 2          # (one more in the library: the handle)
            assert sorted(info) == ["episode_length", "push", "terms", "timeout"]
            assert info["push"].shape == (3, 3) and info["push"].data_ptr() == wc.xfrc.data_ptr() and info["push"].stride() == (18, 1)
        else:
            assert sorted(info) == ["episode_length", "terms", "timeout"]
        if noise:
            rn = by["tsidb_policy_reset_noise"]
            assert len(rn) == 6 and rn[1].value == wc.rows.data_ptr() and rn[2] == wc.NROW
            assert [a.value for a in rn[3:5]] == [wc.qpos.data_ptr(), wc.qvel.data_ptr()]
        assert len(by["tsidb_policy_obs"]) == 8 and len(by["tsidb_policy_act"]) == 3
    # off: today's calls, today's info
    env, calls = bare_env(decimation=4)
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert sorted(info) == ["episode_length", "terms", "timeout"]
    assert _lib.POL_DR_NPARAMS == 23


def test_reset_applies_the_reset_noise_before_the_observation():
    env, calls = bare_env()
    env._dr_reset = True
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_reset_noise", "tsidb_policy_obs"]
    env, calls = bare_env()
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs"]
