"""TSID in the loop of the policy environment (PolicyEnv(tsid=...); tsidb_policy_teacher / _teacher_obs), the parts that need
no GPU: the binding against the header, both libraries' exports, the launches a tsid step makes on a bare env, and the
arguments the constructor rejects before it builds anything."""
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_host import bare_env  # noqa: E402

NAMES = ("tsidb_policy_teacher_config", "tsidb_policy_teacher", "tsidb_policy_teacher_obs")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text, en = HEADER, header_enums("TSIDB_POL_TEACH_")
    assert _lib.POL_TEACH_NT == en["TSIDB_POL_TEACH_NT"] == len(_lib.POL_TEACH_TERMS) == 4
    for k in ("SIGMA_COM", "SIGMA_FOOT", "WEIGHTS", "NPARAMS"):
        assert getattr(_lib, "POL_TEACH_" + k) == en["TSIDB_POL_TEACH_" + k], k
    assert _lib.POL_TEACH_NPARAMS == _lib.POL_TEACH_WEIGHTS + _lib.POL_TEACH_NT == 6
    assert _lib.pol_teach_nobs(20) == en["TSIDB_POL_TEACH_NOBS"] == 34 and _lib.pol_teach_nobs(18) == 32
    # the terms in the header's table order
    table = re.findall(r"^ \*   (track_com|track_feet|contact_match|deviation)\b", text, re.M)
    assert tuple(table) == _lib.POL_TEACH_TERMS
    # the policy parameter vector was not renumbered
    assert (_lib.POL_P_CLIP, _lib.POL_P_WEIGHTS, _lib.POL_NPARAMS) == (0, 15, 27)
    assert_prototypes(NAMES)


def test_class_level_defaults_leave_a_bare_env_without_tsid():
    from tsid_control_amd.policy_env import PolicyEnv
    assert PolicyEnv.tsid is None and PolicyEnv.sched is None and PolicyEnv.clock is None
    env, calls = bare_env(decimation=4)
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert sorted(info) == ["episode_length", "terms", "timeout"]


def tsid_env(tsid, decimation):
    """bare_env with what a tsid step touches: the tick's outputs, the teacher's buffers and, for "walk", a schedule on the host"""
    from tsid_control_amd import RobotConfig, _lib
    from tsid_control_amd.walk_planner import WalkSchedule, op3_closed_loop_walking_conf
    env, calls = bare_env(decimation=decimation)
    wc, n = env.wc, env.num_envs
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    wc.conf, wc.t = op3_closed_loop_walking_conf(RobotConfig()), 0.0
    wc.tau, wc.dv, wc.f, wc.status = z(n, wc.NA), z(n, wc.NV), z(n, 24), z(n, dt=torch.int32)
    wc.obs, wc.com_ref = wc.rows[:, :wc.NOBS], z(n, 9)
    wc.com_ref[:, 2] = 0.24
    env.tsid = tsid
    env.teacher_terms, env.teacher_action, env.teacher_obs = z(n, _lib.POL_TEACH_NT), z(n, wc.NA), z(n, _lib.pol_teach_nobs(wc.NA))
    if tsid == "walk":
        env.clock = z(1)
        env.sched = WalkSchedule.on_device(wc, plan=False, foot_press=0.0, t_start=0.2)
        env.sched.enable_touchdown_feedback()
    return env, calls


def test_stand_step_is_act_step_reward_teacher_reset_obs_teacher_obs():
    env, calls = tsid_env("stand", 10)
    wc = env.wc
    obs, reward, done, info = env.step(torch.zeros(3, wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_step", "tsidb_policy_reward", "tsidb_policy_teacher", "tsidb_reset_done",
                                     "tsidb_policy_obs", "tsidb_policy_teacher_obs"]
    by = {c[0]: c[1] for c in calls}
    assert by["tsidb_step"][-2] == 10                                   # one call, decimation substeps
    te, to = by["tsidb_policy_teacher"], by["tsidb_policy_teacher_obs"]
    assert (len(te), len(to)) == (11, 8)                                # one more in the library: the handle
    assert te[1].value == wc.rows.data_ptr() and te[2] == wc.NROW
    assert [a.value for a in te[3:10]] == [t.data_ptr() for t in (wc.q, wc.tau, wc.status, wc.ncon, wc.con_pairs, env.teacher_terms, env.teacher_action)]
    assert to[1].value == wc.rows.data_ptr() and to[2] == wc.NROW and to[6] == 14 + wc.NA
    assert [a.value for a in to[3:6]] == [t.data_ptr() for t in (wc.qpos, wc.tau, env.teacher_obs)]
    assert sorted(info) == ["episode_length", "teacher_action", "teacher_obs", "teacher_terms", "terms", "timeout"]
    assert info["teacher_terms"] is env.teacher_terms and info["teacher_action"] is env.teacher_action and info["teacher_obs"] is env.teacher_obs
    assert info["teacher_obs"].shape == (3, 34)


def test_walk_step_updates_the_references_before_every_tick_and_replans_after_the_reset():
    env, calls = tsid_env("walk", 4)
    wc = env.wc
    env._dr_reset = True
    env.step(torch.zeros(3, wc.NA, dtype=torch.float64))
    names = [c[0] for c in calls]
    assert names == ["tsidb_policy_act"] + ["tsidb_walk_update", "tsidb_step"] * 4 + \
        ["tsidb_policy_reward", "tsidb_policy_teacher", "tsidb_reset_done", "tsidb_walk_plan", "tsidb_policy_reset_noise", "tsidb_policy_obs",
         "tsidb_policy_teacher_obs"]
    assert float(env.clock) == pytest.approx(4 * wc.conf.dt, abs=1e-15)
    for name, args in calls:
        if name == "tsidb_step":
            assert args[-2] == 1
        if name == "tsidb_walk_update":                                 # the device clock, and the touch-down latch
            assert args[-2] == env.clock.data_ptr() and args[16] == env.sched.td_latch.data_ptr()
    plan = dict(calls)["tsidb_walk_plan"]
    # the done envs only, on a new path, at the device clock
    assert plan[0] is None and plan[2].value == wc.rows.data_ptr() and plan[3] == wc.NROW and plan[11] == 1 and plan[-2].value == env.clock.data_ptr()
    # reset(): the same replanning; a full reset rewinds the clock
    del calls[:]
    env.reset([1])
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_walk_plan", "tsidb_policy_reset_noise", "tsidb_policy_obs", "tsidb_policy_teacher_obs"]
    assert float(env.clock) > 0
    env.reset()
    assert float(env.clock) == 0
    # written(): the clock, the schedule's tables and the teacher's buffers are part of what a captured step rewinds
    wc.ctrl = wc.xfrc = wc._readouts = wc.sensordata = None
    env.act_hist = env.last_action = env.prev_action = env.command = env.air_time = env.episode = None
    for k in ("posture_ref", "foot_ref", "contact_ref", "contact_active", "cop_ref"):
        setattr(wc, k, None)
    ids = {id(t) for t in env.written()}
    s = env.sched
    for t in (env.clock, s.td_latch, s.t_offset, s.coef, s.rest, s.com, s.side, s.nsteps, s.episode, env.teacher_terms, env.teacher_action,
              env.teacher_obs, wc.status, wc.tau):
        assert id(t) in ids


@pytest.mark.parametrize("kw,msg", [
    (dict(mode="residual"), "residual"),
    (dict(tsid="trot"), "tsid must be None, 'stand' or 'walk'"),
    (dict(tsid="stand"), "op3_closed_loop_walking_conf"),
    (dict(tsid="walk", mode="residual"), "op3_closed_loop_walking_conf"),
    (dict(walk=dict(t_start=0.2)), "need tsid"),
    (dict(teacher_weights=dict(track_com=1.0)), "need tsid"),
    (dict(tsid="stand", closed=True, walk=dict(t_start=0.2)), "tsid = 'walk'"),
    (dict(tsid="stand", closed=True, teacher_weights=dict(track_comm=1.0)), "unknown teacher terms"),
    (dict(tsid="stand", closed=True, sigma_com=0.0), "sigma_com"),
    (dict(tsid="walk", closed=True, sigma_com=-0.1), "sigma_com"),
    (dict(tsid="stand", closed=True, sigma_foot=0.0), "sigma_foot"),
    (dict(tsid="stand", closed=True, teacher_weights=dict(deviation=float("nan"))), "non-finite"),
    (dict(tsid="stand", closed=True, randomization=dict(reset_xy=0.1)), "reset_xy"),
    (dict(tsid="walk", closed=True, randomization=dict(reset_yaw=0.5)), "reset_yaw"),
    (dict(tsid="stand", closed=True, randomization=dict(reset_lift=0.01, reset_joint_pos=0.1)), "reset_lift"),
])
def test_rejected_arguments_raise_before_anything_is_built(kw, msg, monkeypatch):
    """every check sits ahead of the controller's construction: a WalkController that raises proves it"""
    from tsid_control_amd import RobotConfig, _lib, policy_env

    def never(*a, **k):
        raise AssertionError("the controller was built before the arguments were checked")

    monkeypatch.setattr(policy_env, "WalkController", never)
    kw = dict(kw)
    conf = RobotConfig()
    conf.closed_loop = bool(kw.pop("closed", False))
    with pytest.raises(_lib.TsidbError, match=msg):
        policy_env.PolicyEnv(conf, num_envs=2, device="cuda:0", **kw)


def test_joint_and_velocity_reset_noise_passes_the_checks():
    """reset noise that leaves the base where the references were captured is allowed with tsid: the constructor gets as far as
    the controller"""
    from tsid_control_amd import RobotConfig, policy_env

    class Built(Exception):
        pass

    def built(*a, **k):
        raise Built()

    conf = RobotConfig()
    conf.closed_loop = True
    keep = policy_env.WalkController
    policy_env.WalkController = built
    try:
        with pytest.raises(Built):
            policy_env.PolicyEnv(conf, num_envs=2, device="cuda:0", tsid="stand", mode="residual",
                                 randomization=dict(reset_joint_pos=0.05, reset_joint_vel=0.1, reset_base_lin_vel=0.1, noise_gravity=0.01))
    finally:
        policy_env.WalkController = keep
