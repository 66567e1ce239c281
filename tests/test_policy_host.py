"""The policy environment (tsidb_policy_* / PolicyEnv), the parts that need no GPU: the binding against the header, both
libraries' exports, and the launches one PolicyEnv.step() makes."""
import ctypes as C
import re
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402

NAMES = ("tsidb_policy_config", "tsidb_policy_act", "tsidb_policy_reward", "tsidb_policy_obs")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text, en = HEADER, header_enums()
    assert (_lib.POL_NT, _lib.POL_HIST, _lib.POL_NPRIV) == (en["TSIDB_POL_NT"], en["TSIDB_POL_HIST"], en["TSIDB_POL_NPRIV"]) == (12, 8, 4)
    assert len(_lib.POL_TERMS) == _lib.POL_NT and len(set(_lib.POL_TERMS)) == _lib.POL_NT
    assert _lib.pol_nobs(en["TSIDB_NA"]) == en["TSIDB_POL_NOBS"] == 71 and _lib.pol_nobs(18) == 65
    for k in ("CLIP", "ALPHA", "SIGMA", "H_TARGET", "T_AIR", "DEADBAND", "MAX_EPISODE_STEPS", "DECIMATION", "SEED", "CMD_LO", "CMD_HI", "WEIGHTS"):
        assert getattr(_lib, "POL_P_" + k) == en["TSIDB_POL_P_" + k], k
    assert _lib.POL_NPARAMS == en["TSIDB_POL_NPARAMS"] == _lib.POL_P_WEIGHTS + _lib.POL_NT
    assert _lib.POL_P_CMD_HI == _lib.POL_P_CMD_LO + 3 and _lib.POL_P_WEIGHTS == _lib.POL_P_CMD_HI + 3
    # the terms in the header's table order
    table = re.findall(r"\b(\d+) (track_lin_vel|track_ang_vel|lin_vel_z|ang_vel_xy|orientation|base_height|torques|action_rate|joint_vel|feet_air_time|alive|termination)\b", text)
    assert sorted((int(i), k) for i, k in table) == list(enumerate(_lib.POL_TERMS))
    # the struct: the header's fields in order, pointers then the stride
    m = re.search(r"typedef struct tsidb_policy_bufs \{(.*?)\} tsidb_policy_bufs;", text, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicyBufs._fields_]
    assert [f[1] for f in _lib.PolicyBufs._fields_] == [C.c_void_p] * 11 + [C.c_int]
    # the prototypes: as many arguments as the header declares, and both libraries export them
    assert_prototypes(NAMES)


def test_policy_env_is_exported():
    import tsid_control_amd
    from tsid_control_amd.policy_env import PolicyEnv
    assert tsid_control_amd.PolicyEnv is PolicyEnv


def bare_env(n=3, decimation=10):
    """a PolicyEnv over a bare WalkController: sizes and tensors (on the CPU), no device, no library handle; every library
    call is recorded"""
    from test_ctrl_host import bare_controller
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyEnv
    wc = bare_controller()
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    wc.num_envs, wc.dtype, wc.device = n, torch.float64, torch.device("cpu")
    wc.NOBS, wc.NROW = wc.NQ + wc.NV + 12, wc.NQ + wc.NV + 14
    wc.q, wc.v, wc.frames = z(n, wc.NQ), z(n, wc.NV), z(n, 2, 12)
    wc.qpos, wc.qvel, wc.qacc_warmstart = z(n, wc.NQ), z(n, wc.NV), z(n, wc.NV)
    wc.ncon, wc.con_pairs, wc.info = z(n, dt=torch.int32), z(n, 32, dt=torch.int32), z(n, 4, dt=torch.int32)
    wc.rows = z(n, wc.NROW)
    wc.reward, wc.done = wc.rows[:, wc.NOBS], wc.rows[:, wc.NOBS + 1]
    calls = []
    wc._call = lambda name, *args: calls.append((name, args))
    wc._stream = lambda: C.c_void_p(0)
    env = object.__new__(PolicyEnv)
    env.wc, env.num_envs, env.NA, env.decimation = wc, n, wc.NA, decimation
    env.NOBS = _lib.pol_nobs(wc.NA)
    env._rows = z(n, env.NOBS + _lib.POL_NPRIV)
    env.obs, env.priv, env.reward, env.done = env._rows[:, :env.NOBS], env._rows[:, env.NOBS:], wc.reward, wc.done
    env.terms, env.timeout, env.ep_len = z(n, _lib.POL_NT), z(n, dt=torch.int32), z(n, dt=torch.int32)
    env._bufs = _lib.PolicyBufs()
    return env, calls


def test_step_is_act_sim_reward_reset_obs():
    for decimation, sims in ((10, [8, 2]), (4, [4]), (16, [8, 8])):
        env, calls = bare_env(decimation=decimation)
        wc = env.wc
        action = torch.zeros(3, wc.NA, dtype=torch.float64)
        obs, reward, done, info = env.step(action)
        names = [c[0] for c in calls]
        assert names == ["tsidb_policy_act"] + ["tsidb_sim_ctrl"] * len(sims) + ["tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
        assert [c[1][0] for c in calls if c[0] == "tsidb_sim_ctrl"] == sims
        by = {c[0]: c[1] for c in calls}
        act, rew, rst, ob = by["tsidb_policy_act"], by["tsidb_policy_reward"], by["tsidb_reset_done"], by["tsidb_policy_obs"]
        # every call carries one more argument (the handle) in the library: the header's counts
        assert (len(act), len(rew), len(ob)) == (3, 10, 8)
        assert act[1].value == action.data_ptr()
        assert [a.value for a in rew[1:6]] == [t.data_ptr() for t in (wc.qpos, wc.qvel, wc.ncon, wc.con_pairs, wc.info)]
        # reward and done land in the columns the reset reads its done flags from, a row apart
        assert rew[6].value == wc.rows.data_ptr() + 8 * wc.NOBS and rew[7].value == wc.rows.data_ptr() + 8 * (wc.NOBS + 1) and rew[8] == wc.NROW
        assert rst[0].value == wc.rows.data_ptr() and rst[1] == wc.NROW
        assert ob[1].value == wc.rows.data_ptr() and ob[2] == wc.NROW and [a.value for a in ob[3:7]] == \
            [t.data_ptr() for t in (wc.qpos, wc.qvel, wc.ncon, wc.con_pairs)]
        assert obs is env.obs and reward is wc.reward and done is wc.done
        assert sorted(info) == ["episode_length", "terms", "timeout"] and info["terms"] is env.terms and info["timeout"] is env.timeout
        assert obs.shape == (3, 71) and env.priv.shape == (3, 4)
