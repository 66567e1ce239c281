"""Episode statistics and the terrain curriculum of the policy environment (tsidb_policy_episode_config / _end / _begin,
PolicyCurriculum, PolicyEnv(episode_stats=, curriculum=)), the parts that need no GPU: the binding against the header, both
libraries' exports, the configurations the host rejects, and the launches a step() / reset() makes with the slice on and off."""
import ctypes as C
import dataclasses
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_episode_reference as er  # noqa: E402
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_host import bare_env  # noqa: E402
from test_policy_terrain_host import terrain_env  # noqa: E402

NAMES = ("tsidb_policy_episode_config", "tsidb_policy_episode_end", "tsidb_policy_episode_begin")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    en = header_enums("TSIDB_POL_EP_")
    cols = ("COUNT", "TIMEOUT", "LENGTH", "RETURN", "DISPLACEMENT", "LEVEL", "TERMS", "TEACH", "NREC")
    assert [en["TSIDB_POL_EP_" + k] for k in cols] == [getattr(_lib, "POL_EP_" + k) for k in cols] == [0, 1, 2, 3, 4, 5, 6, 18, 22]
    assert len(en) == len(cols)
    assert _lib.POL_EP_TEACH == _lib.POL_EP_TERMS + _lib.POL_NT and _lib.POL_EP_NREC == _lib.POL_EP_TEACH + _lib.POL_TEACH_NT
    # the restatement's columns are the header's
    assert [getattr(er, k) for k in cols] == [en["TSIDB_POL_EP_" + k] for k in cols] and (er.NT, er.TEACH_NT) == (_lib.POL_NT, _lib.POL_TEACH_NT)
    en = header_enums("TSIDB_POL_EPP_")
    names = ("CURRICULUM", "UP_DISTANCE", "DOWN_FRACTION", "RANDOM_TOP", "NPARAMS")
    assert [en["TSIDB_POL_EPP_" + k] for k in names] == [getattr(_lib, "POL_EPP_" + k) for k in names] == [0, 1, 2, 3, 4] and len(en) == 5
    # the whole header still evaluates, and the older vectors keep their sizes
    every = header_enums()
    assert every["TSIDB_POL_TER_NPARAMS"] == 23 and every["TSIDB_POL_DR_NPARAMS"] == 23 and every["TSIDB_POL_NPARAMS"] == 27
    # the struct: the header's fields in order, six pointers
    m = re.search(r"typedef struct tsidb_policy_episode \{(.*?)\} tsidb_policy_episode;", HEADER, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicyEpisode._fields_] == ["run", "start_xy", "last", "sum", "level", "teacher_terms"]
    assert [f[1] for f in _lib.PolicyEpisode._fields_] == [C.c_void_p] * 6 and C.sizeof(_lib.PolicyEpisode) == 48
    assert C.sizeof(_lib.PolicyBufs) == 11 * 8 + 8                               # (the env's block did not grow)
    # stream 24 has its row in the key table, behind the teacher / student draw
    assert _lib.POL_CURRICULUM_STREAM == er.STREAM == 24 == _lib.POL_TEACHER_MIX_STREAM + 1
    assert re.search(r"^ \*   24  ", HEADER, re.M)
    assert_prototypes(NAMES)
    # without a handle nothing is looked at
    for lib in sorted((Path(_lib.__file__).parent).glob("libtsidb*.so")):
        L = _lib.load(lib)
        assert L.tsidb_policy_episode_config(None, None, 0) == -1
        assert L.tsidb_policy_episode_end(*([None] * 6), 1, None) == -1
        assert L.tsidb_policy_episode_begin(*([None] * 4), 0, None, None) == -1


def test_curriculum_is_exported_and_its_vector_is_the_librarys():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyCurriculum, PolicyEnv
    assert tsid_control_amd.PolicyCurriculum is PolicyCurriculum
    assert [f.name for f in dataclasses.fields(PolicyCurriculum)] == list(_lib.POL_CURRICULUM_FIELDS)
    assert PolicyEnv.curriculum is None and PolicyEnv._episode is None and PolicyEnv.episode_sum is None and PolicyEnv.episode_last is None
    assert list(PolicyCurriculum(0.4).params()) == [1.0, 0.4, 0.5, 1.0]
    assert list(PolicyCurriculum.of(dict(up_distance=2, down_fraction=0, random_top=False)).params()) == [1.0, 2.0, 0.0, 0.0]
    c = PolicyCurriculum(0.4)
    assert PolicyCurriculum.of(c) is c


@pytest.mark.parametrize("bad,msg", [
    (dict(up_distance=0.0), "up_distance must be positive"), (dict(up_distance=-1.0), "up_distance must be positive"),
    (dict(up_distance=float("nan")), "non-finite"), (dict(up_distance=1.0, down_fraction=float("inf")), "non-finite"),
    (dict(up_distance=1.0, down_fraction=-0.1), "down_fraction must be >= 0"), (dict(up_distance=1.0, random_top=2), "random_top"),
    (dict(up_distance=1.0, random_top="yes"), "random_top"), (dict(up_distance="far"), "not numbers"),
    (dict(up_distance=1.0, up_fraction=0.5), "unknown curriculum fields"),
])
def test_rejected_curricula_raise_with_a_message(bad, msg):
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyCurriculum
    with pytest.raises(_lib.TsidbError, match=msg):
        PolicyCurriculum.of(bad).params()
    with pytest.raises(_lib.TsidbError, match="PolicyCurriculum or a dict"):
        PolicyCurriculum.of(0.5)


def test_a_curriculum_needs_a_terrain_and_an_episode_length():
    """both are checked before anything is built: no device is touched"""
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv
    for kw in (dict(max_episode_steps=6), dict(terrain=dict(num_levels=3)), dict(terrain=dict(num_levels=3), max_episode_steps=0)):
        with pytest.raises(_lib.TsidbError, match="a curriculum needs terrain= .* and max_episode_steps > 0"):
            PolicyEnv(num_envs=2, device="cpu", curriculum=dict(up_distance=0.3), **kw)
    with pytest.raises(_lib.TsidbError, match="up_distance must be positive"):
        PolicyEnv(num_envs=2, device="cpu", terrain=dict(num_levels=3), max_episode_steps=6, curriculum=dict(up_distance=0.0))
    env, _ = bare_env()
    with pytest.raises(_lib.TsidbError, match="built without episode_stats"):
        env.episode_stats()


def episode_env(decimation=4, terrain=False, curriculum=False):
    """bare_env / terrain_env with the slice on"""
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyCurriculum
    env, calls = terrain_env(decimation) if terrain else bare_env(decimation=decimation)
    d = lambda *s: torch.zeros(*s, dtype=torch.float64)
    env.episode_run, env.episode_start_xy, env.episode_last, env.episode_sum = d(3, 22), d(3, 2), d(3, 22), d(3, 22)
    env._episode = _lib.PolicyEpisode()
    if curriculum:
        env.curriculum = PolicyCurriculum(0.3)
    return env, calls


def test_step_and_reset_with_the_slice_on():
    env, calls = episode_env()
    wc = env.wc
    obs, reward, done, info = env.step(torch.zeros(3, wc.NA, dtype=torch.float64))
    names = [c[0] for c in calls]
    assert names == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_policy_episode_end", "tsidb_reset_done",
                     "tsidb_policy_episode_begin", "tsidb_policy_obs"]
    by = {c[0]: c[1] for c in calls}
    end, begin = by["tsidb_policy_episode_end"], by["tsidb_policy_episode_begin"]
    assert len(end) == 7 and len(begin) == 6                          # (one more in the library: the handle)
    assert end[2].value == wc.qpos.data_ptr() and end[3].value == wc.reward.data_ptr() and end[4].value == wc.done.data_ptr() and end[5] == wc.NROW
    assert begin[2].value == wc.rows.data_ptr() and begin[3] == wc.NROW and begin[4].value == wc.qpos.data_ptr()
    assert sorted(info) == ["episode_last", "episode_length", "episode_sum", "terms", "timeout"]
    assert info["episode_last"] is env.episode_last and info["episode_sum"] is env.episode_sum
    # reset(): the episodes it forces start, nothing is recorded for the ones it abandons
    env, calls = episode_env()
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_episode_begin", "tsidb_policy_obs"]
    # with a terrain and reset noise: end directly before the reset, begin behind the terrain's redraw
    env, calls = episode_env(terrain=True, curriculum=True)
    env._dr_reset = True
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    names = [c[0] for c in calls]
    assert names[2:] == ["tsidb_policy_reward", "tsidb_policy_episode_end", "tsidb_reset_done", "tsidb_policy_reset_noise",
                         "tsidb_policy_terrain_reset", "tsidb_policy_episode_begin", "tsidb_policy_obs", "tsidb_policy_height_scan"]
    assert sorted(info) == ["env_params", "episode_last", "episode_length", "episode_sum", "height_scan", "terms", "terrain_level", "timeout"]
    env, calls = episode_env(terrain=True, curriculum=True)
    env._dr_reset = True
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_reset_noise", "tsidb_policy_terrain_reset", "tsidb_policy_episode_begin",
                                     "tsidb_policy_obs", "tsidb_policy_height_scan"]


def test_step_with_tsid_puts_the_end_behind_the_teacher():
    from test_policy_tsid_host import tsid_env
    from tsid_control_amd import _lib
    env, calls = tsid_env("stand", 4)
    d = lambda *s: torch.zeros(*s, dtype=torch.float64)
    env.episode_run, env.episode_start_xy, env.episode_last, env.episode_sum = d(3, 22), d(3, 2), d(3, 22), d(3, 22)
    env._episode = _lib.PolicyEpisode()
    del calls[:]
    env.step(torch.zeros(env.num_envs, env.NA, dtype=torch.float64))
    names = [c[0] for c in calls]
    i = names.index("tsidb_policy_episode_end")
    assert names[i - 1] == "tsidb_policy_teacher" and names[i + 1] == "tsidb_reset_done"
    assert names.index("tsidb_policy_episode_begin") > i + 1


def test_off_is_todays_calls_info_and_written():
    env, calls = bare_env(decimation=4)
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert sorted(info) == ["episode_length", "terms", "timeout"]
    env, calls = bare_env()
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs"]
    env, calls = terrain_env()
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert not any("episode" in c[0] for c in calls)
    assert sorted(info) == ["env_params", "episode_length", "height_scan", "terms", "terrain_level", "timeout"]


def written_ids(env):
    """ids of the tensors written() yields behind the controller's own"""
    env.wc._written = lambda: iter(())
    for k in ("ctrl", "xfrc"):
        if not hasattr(env.wc, k):
            setattr(env.wc, k, None)
    for k in ("act_hist", "last_action", "prev_action", "command", "air_time", "episode"):
        if not hasattr(env, k):
            setattr(env, k, torch.zeros(1))
    return [id(t) for t in env.written() if t is not None]


def test_written_yields_the_new_tensors_only_while_the_slice_is_on():
    off, _ = terrain_env()
    on, _ = episode_env(terrain=True)
    cur, _ = episode_env(terrain=True, curriculum=True)
    n_off, ids_on, ids_cur = len(written_ids(off)), written_ids(on), written_ids(cur)
    new = [id(t) for t in (on.episode_run, on.episode_start_xy, on.episode_last, on.episode_sum)]
    assert ids_on[n_off:] == new and len(ids_on) == n_off + 4 and id(on.terrain_level) not in ids_on
    assert len(ids_cur) == n_off + 5 and ids_cur[-1] == id(cur.terrain_level)
    assert id(off.terrain_level) not in written_ids(off)


def test_episode_stats_are_the_means_of_the_sums():
    from tsid_control_amd import _lib
    env, _ = episode_env()
    rng = np.random.default_rng(0)
    s = rng.uniform(0.0, 3.0, (3, 22))
    s[:, 0], s[:, 1] = [2, 0, 3], [1, 0, 1]
    env.episode_sum.copy_(torch.as_tensor(s))
    out = env.episode_stats(clear=False)
    keys = ["episodes", "timeouts", "length", "return", "displacement", "level"] + ["rew_" + k for k in _lib.POL_TERMS]
    assert list(out) == keys and all(v.dim() == 0 and v.dtype == torch.float64 for v in out.values())
    tot = s.sum(0)
    assert float(out["episodes"]) == 5 and float(out["timeouts"]) == 2
    assert np.allclose([float(out[k]) for k in keys[2:]], tot[2:18] / 5, rtol=1e-15)
    assert float(env.episode_sum.sum()) != 0
    env.tsid = "stand"
    out = env.episode_stats()
    assert list(out) == keys + ["teacher_" + k for k in _lib.POL_TEACH_TERMS] and float(env.episode_sum.abs().sum()) == 0
    assert np.allclose([float(out["teacher_" + k]) for k in _lib.POL_TEACH_TERMS], tot[18:] / 5, rtol=1e-15)
    # nothing finished: the divisor is 1
    out = env.episode_stats()
    assert all(float(v) == 0 for v in out.values())
