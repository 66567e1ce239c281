"""Per-episode terrain and dynamics of the policy environment and its height scan (tsidb_policy_terrain_config / _terrain_reset /
_height_scan, PolicyTerrain), the parts that need no GPU: the binding against the header, both libraries' exports, the
configurations the host rejects, and the launches a PolicyEnv.step() / reset() with a terrain makes."""
import dataclasses
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_host import bare_env  # noqa: E402

NAMES = ("tsidb_policy_terrain_config", "tsidb_policy_terrain_reset", "tsidb_policy_height_scan")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text, en = HEADER, header_enums("TSIDB_POL_TER_")
    assert len(en) == len(_lib.POL_TER_NAMES) + 1 == 24
    for k in _lib.POL_TER_NAMES:
        assert getattr(_lib, "POL_TER_" + k.upper()) == en["TSIDB_POL_TER_" + k.upper()], k
    assert _lib.POL_TER_NPARAMS == en["TSIDB_POL_TER_NPARAMS"] == 23
    assert _lib.POL_MAXSCAN == int(re.search(r"TSIDB_POL_MAXSCAN = (\d+)", text).group(1)) == 256
    # the randomisation's vector and the observation keep their sizes
    assert _lib.POL_DR_NPARAMS == 23 and _lib.pol_nobs(20) == 71 and _lib.POL_NPRIV == 4
    # the streams continue the header's table
    for stream in range(12, 21):
        assert re.search(r"^ \*   %d  " % stream, text, re.M), stream
    assert_prototypes(NAMES)


def test_terrain_is_exported_and_its_defaults_are_the_nominal_floor():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv, PolicyTerrain
    assert tsid_control_amd.PolicyTerrain is PolicyTerrain
    assert [f.name for f in dataclasses.fields(PolicyTerrain)] == list(_lib.POL_TER_FIELDS)
    assert PolicyEnv.terrain is None and PolicyEnv.terrain_level is None and PolicyEnv.height_scan is None
    p = PolicyTerrain().params(default_seed=5, default_env_offset=16)
    want = dict(seed=5, env_offset=16, mass_lo=1, mass_hi=1, friction_lo=1, friction_hi=1, step_length_lo=0.08, step_length_hi=0.08,
                step_prob=0.5, flat_cells=1, num_levels=1, scan_clip_lo=-1, scan_clip_hi=1)
    assert p.shape == (_lib.POL_TER_NPARAMS,)
    assert {k: p[i] for i, k in enumerate(_lib.POL_TER_NAMES)} == {k: float(want.get(k, 0)) for k in _lib.POL_TER_NAMES}
    p = PolicyTerrain.of(dict(seed=2, env_offset=4, mass=(0.98, 1.02), friction=(0.4, 1.0), tilt_deg=5.0, step_height=(0.0, 0.01),
                              step_length=(0.04, 0.12), num_levels=3, scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7), scan_clip=(-0.2, 0.6),
                              scan_noise=0.01)).params(default_seed=9)
    assert p[_lib.POL_TER_SEED] == 2 and p[_lib.POL_TER_ENV_OFFSET] == 4 and p[_lib.POL_TER_TILT_MAX] == math.radians(5.0)
    assert list(p[_lib.POL_TER_SCAN_NX:_lib.POL_TER_SCAN_Y1 + 1]) == [11, 7, -0.5, 0.5, -0.3, 0.3]
    assert list(p[_lib.POL_TER_SCAN_CLIP_LO:]) == [-0.2, 0.6, 0.01] and list(p[_lib.POL_TER_STEP_HEIGHT_LO:_lib.POL_TER_STEP_PROB]) == [0.0, 0.01, 0.04, 0.12]
    assert PolicyTerrain(scan_x=(0, 1, 16), scan_y=(0, 1, 16)).params()[_lib.POL_TER_SCAN_NX] == 16      # 256 points: the most


@pytest.mark.parametrize("bad,msg", [
    (dict(tilt_deg=float("nan")), "non-finite"), (dict(mass=(1.0, float("inf"))), "non-finite"),
    (dict(mass=(1.1, 0.9)), "mass: lo > hi"), (dict(friction=(1.0, 0.5)), "friction: lo > hi"), (dict(step_height=(0.02, 0.01)), "step_height: lo > hi"),
    (dict(step_length=(0.2, 0.1)), "step_length: lo > hi"), (dict(scan_clip=(1.0, -1.0)), "scan_clip: lo > hi"),
    (dict(mass=(0.0, 1.0)), "mass must be positive"), (dict(friction=(-0.1, 1.0)), "friction must be positive"),
    (dict(tilt_deg=45.0), r"\[0, 45\)"), (dict(tilt_deg=-1.0), r"\[0, 45\)"), (dict(step_height=(-0.01, 0.01)), "step_height must be >= 0"),
    (dict(step_length=(0.0, 0.1)), "step_length must be positive"), (dict(step_prob=1.5), r"\[0, 1\]"), (dict(step_prob=-0.1), r"\[0, 1\]"),
    (dict(flat_cells=1.5), "flat_cells"), (dict(flat_cells=8), "flat_cells"), (dict(flat_cells=-1), "flat_cells"),
    (dict(num_levels=0), "num_levels"), (dict(num_levels=2.5), "num_levels"),
    (dict(seed=2 ** 32), "seed"), (dict(seed=0.5), "seed"), (dict(env_offset=2 ** 31), "env_offset"), (dict(env_offset=-1), "env_offset"),
    (dict(scan_x=(0, 1, 17), scan_y=(0, 1, 16)), "at most 256"), (dict(scan_x=(0, 1, 3)), "both"), (dict(scan_x=(0, 1, 3), scan_y=(0, 1, 0)), "both"),
    (dict(scan_x=(0, 1, 2.5), scan_y=(0, 1, 2)), "scan_nx"), (dict(scan_x=(0, 1), scan_y=(0, 1, 2)), "scan_x"),
    (dict(scan_noise=-0.01), "scan_noise"), (dict(mass=1.0), "mass"), (dict(step_prob="half"), "step_prob"),
    (dict(step_hieght=(0.0, 0.01)), "unknown terrain fields"),
])
def test_rejected_configurations_raise_with_a_message(bad, msg):
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyTerrain
    with pytest.raises(_lib.TsidbError, match=msg):
        PolicyTerrain.of(bad).params()
    with pytest.raises(_lib.TsidbError, match="PolicyTerrain or a dict"):
        PolicyTerrain.of([1, 2, 3])


def terrain_env(decimation=4, points=77):
    from tsid_control_amd.policy_env import PolicyTerrain
    env, calls = bare_env(decimation=decimation)
    wc = env.wc
    wc.env_params, wc.terrain = torch.zeros(3, 8, dtype=torch.float64), torch.zeros(3, 20, dtype=torch.float64)
    env.terrain = PolicyTerrain()
    env.terrain_level = torch.zeros(3, dtype=torch.int32)
    env.height_scan = torch.zeros(3, points, dtype=torch.float64)
    return env, calls


def test_step_with_a_terrain_is_act_sim_reward_reset_terrain_obs_scan():
    env, calls = terrain_env()
    wc = env.wc
    obs, reward, done, info = env.step(torch.zeros(3, wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done",
                                     "tsidb_policy_terrain_reset", "tsidb_policy_obs", "tsidb_policy_height_scan"]
    by = {c[0]: c[1] for c in calls}
    tr, sc = by["tsidb_policy_terrain_reset"], by["tsidb_policy_height_scan"]
    assert len(tr) == 6 and len(sc) == 5                         # (one more in the library: the handle)
    assert tr[1].value == wc.rows.data_ptr() and tr[2] == wc.NROW and tr[3].value == wc.qpos.data_ptr() and tr[4].value == env.terrain_level.data_ptr()
    assert sc[1].value == wc.qpos.data_ptr() and sc[2].value == env.height_scan.data_ptr() and sc[3] == 77
    assert sorted(info) == ["env_params", "episode_length", "height_scan", "terms", "terrain_level", "timeout"]
    assert info["height_scan"] is env.height_scan and info["env_params"] is wc.env_params and info["terrain_level"] is env.terrain_level
    # with the reset noise: behind it, so that the plane and cell 0 sit under the randomised position
    env, calls = terrain_env()
    env._dr_reset = True
    env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls][3:] == ["tsidb_reset_done", "tsidb_policy_reset_noise", "tsidb_policy_terrain_reset", "tsidb_policy_obs",
                                         "tsidb_policy_height_scan"]
    # reset(): the same places
    env, calls = terrain_env()
    env._dr_reset = True
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_reset_noise", "tsidb_policy_terrain_reset", "tsidb_policy_obs",
                                     "tsidb_policy_height_scan"]
    # off: today's calls, today's info
    env, calls = bare_env(decimation=4)
    obs, reward, done, info = env.step(torch.zeros(3, env.wc.NA, dtype=torch.float64))
    assert [c[0] for c in calls] == ["tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert sorted(info) == ["episode_length", "terms", "timeout"]
    env, calls = bare_env()
    env.reset()
    assert [c[0] for c in calls] == ["tsidb_reset_done", "tsidb_policy_obs"]


def test_set_env_params_registers_a_flat_terrain_table():
    from test_ctrl_host import bare_controller
    from tsid_control_amd import _lib
    wc = bare_controller()
    calls = []
    wc.num_envs, wc.dtype, wc.device = 4, torch.float64, torch.device("cpu")
    wc._call = lambda name, *args: calls.append((name, args))
    wc.sync_sim = lambda: None
    wc.set_env_params(mass_scale=1.0, terrain="flat")
    assert (wc.env_params == torch.tensor([1.0, 1, 0, 0, 1, 0, 0, 0], dtype=torch.float64)).all() and wc.env_params.shape == (4, 8)
    assert wc.terrain.shape == (4, 20) and (wc.terrain[:, 3] == 1).all() and float(wc.terrain.sum()) == 4.0
    assert calls[-1][0] == "tsidb_set_env_params" and [a.value for a in calls[-1][1]] == [wc.env_params.data_ptr(), wc.terrain.data_ptr()]
    with pytest.raises(_lib.TsidbError, match="'flat'"):
        wc.set_env_params(terrain="hilly")
    assert np.isfinite(wc.terrain.numpy()).all()
