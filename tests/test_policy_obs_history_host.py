"""The observation history of the policy environment (tsidb_policy_obs_history, PolicyObsHistory, PolicyEnv(obs_history=),
"obs_history" as an input block of a PolicyActor), the parts that need no GPU: the binding against the header, both libraries'
exports, the configurations the host rejects, and the launches a step() / reset() makes with the history on and off."""
import ctypes as C
import dataclasses
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_obs_history_reference as hr  # noqa: E402
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_actor_host import actor_env, mlp  # noqa: E402
from test_policy_host import bare_env  # noqa: E402

NAMES = ("tsidb_policy_obs_history",)


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    en = header_enums("TSIDB_POL_OBSH_")
    assert en == dict(TSIDB_POL_OBSH_MAXSRC=4, TSIDB_POL_OBSH_MAXFRAMES=32, TSIDB_POL_OBSH_MAXCOLS=4096)
    assert (_lib.POL_OBSH_MAXSRC, _lib.POL_OBSH_MAXFRAMES, _lib.POL_OBSH_MAXCOLS) == (4, 32, 4096) == (hr.MAXSRC, hr.MAXFRAMES, hr.MAXCOLS)
    assert _lib.POL_OBSH_SOURCES == hr.SOURCES
    assert header_enums()["TSIDB_POL_HIST"] == _lib.POL_HIST == 8                # (the action ring keeps its prefix and its size)
    # the struct: the header's fields in order; it shares its name with the entry point, so it has no typedef
    m = re.search(r"\nstruct tsidb_policy_obs_history \{(.*?)\};", HEADER, re.S)
    fields = re.findall(r"\b(\w+)(?:\[TSIDB_POL_OBSH_MAXSRC\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicyObsHistory._fields_] == ["history", "frames", "n_src", "src", "src_ld", "src_cols"]
    assert [f[1] for f in _lib.PolicyObsHistory._fields_] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p * 4, C.c_int * 4, C.c_int * 4]
    assert C.sizeof(_lib.PolicyObsHistory) == 8 + 4 + 4 + 32 + 16 + 16
    assert C.sizeof(_lib.PolicyBufs) == 11 * 8 + 8                               # (the env's block did not grow)
    assert "const struct tsidb_policy_obs_history *hist" in HEADER
    assert_prototypes(NAMES)
    # without a handle nothing is looked at
    for lib in sorted((Path(_lib.__file__).parent).glob("libtsidb*.so")):
        assert _lib.load(lib).tsidb_policy_obs_history(None, None, None, 0, 1, None) == -1


def test_obs_history_is_exported_and_off_by_default():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv, PolicyObsHistory
    assert tsid_control_amd.PolicyObsHistory is PolicyObsHistory
    assert [f.name for f in dataclasses.fields(PolicyObsHistory)] == list(_lib.POL_OBSH_FIELDS)
    assert PolicyEnv.obs_history is None and PolicyEnv._obs_history is None
    h = PolicyObsHistory(frames=3)
    assert PolicyObsHistory.of(h) is h and h.sources == ("obs",)
    assert PolicyObsHistory.of(dict(frames=2, sources=("command",))).sources == ("command",)
    # the resolution is the restatement's
    cols = dict(obs=71, priv=4, command=3, height_scan=6, teacher_obs=34)
    for sources in (("obs",), "obs", ("obs", "priv"), (("obs", 0, 6), ("obs", 9, 71)), ("command", "height_scan", ("teacher_obs", 3, 5), "priv")):
        assert PolicyObsHistory(2, sources).resolve(cols) == hr.resolve(sources, cols)
    assert PolicyObsHistory(32, (("obs", 0, 64), "priv", ("obs", 0, 60))).resolve(cols)[2] == ("obs", 0, 60)   # 32 x 128 = the cap


REJECTED = [
    (dict(frames=0), "frames must be a whole number in 1 .. 32"),
    (dict(frames=33), "frames must be a whole number in 1 .. 32"),
    (dict(frames=2.5), "frames must be a whole number in 1 .. 32"),
    (dict(frames=True), "frames must be a whole number in 1 .. 32"),
    (dict(frames=2, sources=("observation",)), "unknown source 'observation'"),
    (dict(frames=2, sources=(("obs", 0),)), "unknown source"),
    (dict(frames=2, sources=(("obs", 60, 72),)), r"column range \(60, 72\) of obs"),
    (dict(frames=2, sources=(("priv", 2, 2),)), r"column range \(2, 2\) of priv"),
    (dict(frames=2, sources=(("command", -1, 2),)), r"column range \(-1, 2\) of command"),
    (dict(frames=2, sources=(("obs", 0.0, 6),)), "column range"),
    (dict(frames=2, sources=()), "sources must be a list of 1 .. 4 entries"),
    (dict(frames=2, sources=("obs",) * 5), "sources must be a list of 1 .. 4 entries"),
    (dict(frames=32, sources=("obs", "obs")), "frames . K = 4544 columns, at most 4096"),
    (dict(frames=2, sources=("height_scan",)), "the env has no height_scan .*terrain= with scan_x and scan_y"),
    (dict(frames=2, sources=("obs", "teacher_obs")), "the env has no teacher_obs .*tsid"),
]


@pytest.mark.parametrize("bad,msg", REJECTED)
def test_rejected_configurations_raise_before_a_device_is_touched(bad, msg):
    """device = "cpu": the controller would refuse it, but the history is checked first"""
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv, PolicyObsHistory
    for arg in (bad, PolicyObsHistory(**bad)):
        with pytest.raises(_lib.TsidbError, match="PolicyObsHistory: " + msg):
            PolicyEnv(num_envs=2, device="cpu", obs_history=arg)


def test_more_rejections():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv
    with pytest.raises(_lib.TsidbError, match="obs_history must be a PolicyObsHistory or a dict"):
        PolicyEnv(num_envs=2, device="cpu", obs_history=3)
    with pytest.raises(_lib.TsidbError, match="unknown obs_history fields"):
        PolicyEnv(num_envs=2, device="cpu", obs_history=dict(frames=2, stride=2))
    # a terrain without a scan has no height_scan either; an accepted history gets as far as the controller
    with pytest.raises(_lib.TsidbError, match="the env has no height_scan"):
        PolicyEnv(num_envs=2, device="cpu", terrain=dict(num_levels=2), obs_history=dict(frames=2, sources=("height_scan",)))
    for kw in (dict(obs_history=dict(frames=32, sources=(("obs", 0, 71), ("obs", 0, 57)))),
               dict(terrain=dict(scan_x=(0.0, 0.1, 2), scan_y=(0.0, 0.0, 1)), obs_history=dict(frames=2, sources=("height_scan", ("height_scan", 1, 2))))):
        with pytest.raises(_lib.TsidbError, match="WalkController needs a ROCm device"):
            PolicyEnv(num_envs=2, device="cpu", **kw)


def history_env(frames=3, sources=(("obs", 0, 6), "priv", "command"), decimation=4):
    """bare_env with the history on, built by the env's own _build_obs_history"""
    from tsid_control_amd.policy_env import PolicyObsHistory
    env, calls = bare_env(decimation=decimation)
    env.command = torch.zeros(env.num_envs, 3, dtype=torch.float64)
    env.height_scan = None
    env.obs_history_spec = PolicyObsHistory(frames, sources)
    env.obs_history_sources = env.obs_history_spec.resolve(dict(obs=env.NOBS, priv=4, command=3, height_scan="none", teacher_obs="none"))
    env._build_obs_history()
    return env, calls


def test_the_block_points_into_the_envs_tensors():
    env, _ = history_env()
    h, NOBS = env._obs_history, env.NOBS
    assert (h.frames, h.n_src) == (3, 3) and env.obs_history.shape == (3, 3 * 13) and env.obs_history.dtype == torch.float64
    assert h.history == env.obs_history.data_ptr() and env.obs_history.is_contiguous()
    assert list(h.src)[:3] == [env.obs.data_ptr(), env.priv.data_ptr(), env.command.data_ptr()] and h.src[3] is None
    assert list(h.src_ld) == [NOBS + 4, NOBS + 4, 3, 0] and list(h.src_cols) == [6, 4, 3, 0]
    env, _ = history_env(2, (("obs", 0, 6), ("obs", 9, 71), ("priv", 1, 3)))
    h = env._obs_history
    assert list(h.src)[:3] == [env.obs.data_ptr(), env.obs.data_ptr() + 8 * 9, env.priv.data_ptr() + 8]
    assert list(h.src_cols)[:3] == [6, 62, 2] and env.obs_history.shape == (3, 2 * 70)


def test_step_pushes_and_reset_only_fills():
    env, calls = history_env()
    wc = env.wc
    obs, reward, done, info = env.step(torch.zeros(3, wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs",
                                     "tsidb_policy_obs_history"]
    args = calls[-1][1]
    assert len(args) == 5                                              # (one more in the library: the handle)
    assert C.addressof(args[0]._obj) == C.addressof(env._obs_history) and args[1].value == wc.rows.data_ptr() and args[2] == wc.NROW
    assert args[3] == 1
    assert sorted(info) == ["episode_length", "obs_history", "terms", "timeout"] and info["obs_history"] is env.obs_history
    del calls[:]
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs", "tsidb_policy_obs_history"] and calls[-1][1][3] == 0
    del calls[:]
    env.reset([1])
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs", "tsidb_policy_obs_history"] and calls[-1][1][3] == 0


def test_the_history_is_the_last_launch_of_every_group():
    """behind the height scan and the teacher's observation, which may be its sources"""
    from test_policy_terrain_host import terrain_env
    from test_policy_tsid_host import tsid_env
    from tsid_control_amd import _lib
    env, calls = terrain_env()
    env._obs_history, env.obs_history = _lib.PolicyObsHistory(), torch.zeros(1)
    env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls][-3:] == ["tsidb_policy_obs", "tsidb_policy_height_scan", "tsidb_policy_obs_history"]
    env, calls = tsid_env("stand", 4)
    env._obs_history, env.obs_history = _lib.PolicyObsHistory(), torch.zeros(1)
    del calls[:]
    env.step(torch.zeros(env.num_envs, env.NA, dtype=torch.float64))
    assert [c[0] for c in calls][-3:] == ["tsidb_policy_obs", "tsidb_policy_teacher_obs", "tsidb_policy_obs_history"]


def test_off_is_the_parents_calls_info_and_written():
    from test_policy_episode_host import written_ids
    env, calls = bare_env(decimation=4)
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert sorted(info) == ["episode_length", "terms", "timeout"]
    env, calls = bare_env()
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs"]
    assert env.obs_history is None and env._obs_history is None
    # written(): the history tensor, last, only while it is on
    off, _ = bare_env()
    on, _ = history_env()
    ids_off, ids_on = written_ids(off), written_ids(on)
    assert len(ids_on) == len(ids_off) + 1 and ids_on[-1] == id(on.obs_history)


def test_policy_actor_takes_the_history_as_a_block():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_actor import PolicyActor, _INPUT_NAMES
    assert "obs_history" in _INPUT_NAMES
    env, calls = actor_env()
    NA = env.NA
    with pytest.raises(_lib.TsidbError, match="PolicyActor: actor_inputs: the env has no obs_history .*obs_history="):
        PolicyActor(env, mlp(71, NA), actor_inputs=("obs_history",))
    env.obs_history = torch.zeros(3, 7 * 71, dtype=torch.float64)
    pa = PolicyActor(env, mlp(497 + 3, 8, NA), mlp(497 + 4, 8, 1), actor_inputs=("obs_history", "command"), critic_inputs=("obs_history", "priv"))
    a, c = pa.actor_net.struct, pa.critic_net.struct
    assert list(a.block)[:2] == [env.obs_history.data_ptr(), env.command.data_ptr()] and list(a.block_ld)[:2] == [497, 3]
    assert list(a.block_cols)[:2] == [497, 3] and c.block[0] == env.obs_history.data_ptr() and c.block_cols[1] == 4
    assert pa.actor_input.shape == (3, 500)
    # 8 x 71 is the env's to accept and the actor's to refuse
    env.obs_history = torch.zeros(3, 8 * 71, dtype=torch.float64)
    with pytest.raises(_lib.TsidbError, match="PolicyActor: actor_inputs: the input row has 568 columns, 1 .. 512 allowed"):
        PolicyActor(env, mlp(568, NA), actor_inputs=("obs_history",))
