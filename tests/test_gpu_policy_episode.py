"""Episode statistics and the terrain curriculum on the GPU (tsidb_policy_episode_end / _begin; PolicyEnv(episode_stats=,
curriculum=)): (a) the two entries driven directly on the synthetic scenarios of tests/policy_episode_reference.py, which make
every branch occur, against the numpy restatement; (b) the slice in the env - the restatement on the device's own per-step
buffers, off-is-off and hand-written levels against twins, a captured step, episode_stats() and rollout().

Gates.  level and the COUNT, TIMEOUT, LENGTH and LEVEL columns: exact.  Every other float64 output: 1e-12 relative
(policy_testlib.rel) - the sums are float64 additions of the same addends in the same order on both sides (exact), the
displacement is a product-then-add that may contract to an FMA and a square root: a few ulp.  Rows of envs that were not done:
bit for bit.  No displacement of a scenario lies within 1e-6 m of a threshold, so both paths decide every level alike."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_episode_reference as er  # noqa: E402
from policy_testlib import capture, conf_of, host, make_env, rel, same  # noqa: E402
from test_gpu_policy_dr import CMD, driven  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = [er.COUNT, er.TIMEOUT, er.LENGTH, er.LEVEL]
ROBOTS = [("f64", False), ("f64", True), ("f32", False), ("f32", True)]
T_EPISODE = 500 * (10 * 0.002)      # max_episode_steps * (decimation * dt) of the env behind Direct, as the library forms it
vp = C.c_void_p


def t_episode(env):
    from tsid_control_amd import _lib
    from tsid_control_amd.params import P_DT
    return env.params[_lib.POL_P_MAX_EPISODE_STEPS] * (env.params[_lib.POL_P_DECIMATION] * env.wc.params[P_DT])


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def compare(got, want, err):
    """records [n, NREC]: the exact columns exact, the others into err"""
    assert np.array_equal(got[:, EXACT], want[:, EXACT])
    err[0] = max(err[0], rel(got, want))


# ---------------------------------------------------------------------------- (a) the entries on the scenarios
class Direct:
    """the two entries on buffers of the test's own, with the handle of a configured env"""

    def __init__(self, sc, dtype, v0, curriculum=True, level=True):
        from tsid_control_amd import _lib
        cur = sc["curriculum"]
        n = sc["n"]
        self.env = env = make_env(n, dtype, v0, decimation=10, max_episode_steps=500,
                                  terrain=dict(seed=cur["seed"], env_offset=cur["env_offset"], num_levels=sc["num_levels"]),
                                  curriculum=dict(up_distance=cur["up_distance"], down_fraction=cur["down_fraction"], random_top=cur["random_top"]))
        assert t_episode(env) == cur["t_episode"]
        wc = self.wc = env.wc
        if not curriculum:
            off = np.zeros(_lib.POL_EPP_NPARAMS)
            wc._call("tsidb_policy_episode_config", off.ctypes.data_as(vp), len(off))
        z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
        self.command, self.terms, self.tt = z(n, 3), z(n, _lib.POL_NT), z(n, _lib.POL_TEACH_NT) if sc["teacher"] else None
        self.ep_len, self.episode, self.timeout = z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.int32)
        self.bufs = _lib.PolicyBufs(env.act_hist.data_ptr(), env.last_action.data_ptr(), env.prev_action.data_ptr(), self.command.data_ptr(),
                                    env.air_time.data_ptr(), self.ep_len.data_ptr(), self.episode.data_ptr(), None, self.terms.data_ptr(),
                                    self.timeout.data_ptr(), None, 0)
        self.run, self.start_xy = z(n, er.NREC, dt=torch.float64), z(n, 2, dt=torch.float64)
        self.last, self.sum = z(n, er.NREC, dt=torch.float64), z(n, er.NREC, dt=torch.float64)
        self.level = torch.as_tensor(sc["level0"], device=wc.device).clone() if level else None
        self.ep = _lib.PolicyEpisode(self.run.data_ptr(), self.start_xy.data_ptr(), self.last.data_ptr(), self.sum.data_ptr(),
                                     self.level.data_ptr() if level else None, self.tt.data_ptr() if self.tt is not None else None)
        self.rows, self.qpos = z(n, wc.NROW), z(n, wc.NQ)
        self.qpos[:, 3] = 1
        self.up = lambda a: torch.as_tensor(a, device=wc.device)

    def begin(self, done, xy):
        wc = self.wc
        self.rows[:, wc.NROW - 1] = self.up(done).to(wc.dtype)
        self.qpos[:, :2] = self.up(xy)
        wc._call("tsidb_policy_episode_begin", C.byref(self.bufs), C.byref(self.ep), vp(self.rows.data_ptr()), wc.NROW, vp(self.qpos.data_ptr()),
                 wc._stream())
        torch.cuda.synchronize()

    def end(self, call):
        wc = self.wc
        for t, k in ((self.terms, "terms"), (self.command, "command"), (self.ep_len, "ep_len"), (self.episode, "episode"), (self.timeout, "timeout")):
            t.copy_(self.up(call[k]))
        if self.tt is not None:
            self.tt.copy_(self.up(call["teacher_terms"]))
        self.rows[:, wc.NROW - 2], self.rows[:, wc.NROW - 1] = self.up(call["reward"]), self.up(call["done"])
        self.qpos[:, :2] = self.up(call["xy"])
        wc._call("tsidb_policy_episode_end", C.byref(self.bufs), C.byref(self.ep), vp(self.qpos.data_ptr()),
                 vp(self.rows.data_ptr() + (wc.NROW - 2) * self.rows.element_size()), vp(self.rows.data_ptr() + (wc.NROW - 1) * self.rows.element_size()),
                 wc.NROW, wc._stream())
        torch.cuda.synchronize()

    def play(self, sc, played, err):
        """the scenario call by call against the restatement's record of it; returns every output of every call (bytes)"""
        n, trace = sc["n"], []
        self.begin(np.ones(n), sc["start_xy0"])
        assert np.array_equal(host(self.start_xy), sc["start_xy0"].astype(np.float64)) and not host(self.run).any()
        for call, want in zip(sc["calls"], played):
            fresh = call["done"] != 0
            last0 = host(self.last)
            self.end(call)
            run, last, total = host(self.run), host(self.last), host(self.sum)
            assert bits(last[~fresh]) == bits(last0[~fresh])                          # not done: last untouched, bit for bit
            compare(last, want["last"], err)
            compare(total, want["sum"], err)
            err[0] = max(err[0], rel(run, want["run_end"]))
            assert np.array_equal(run[:, [er.COUNT, er.TIMEOUT, er.DISPLACEMENT, er.LEVEL]], np.zeros((n, 4)))
            if self.level is not None:
                assert np.array_equal(host(self.level), want["level"])
            start0 = host(self.start_xy)
            self.begin(call["done"], call["begin_xy"])
            run1, start1 = host(self.run), host(self.start_xy)
            assert bits(run1[~fresh]) == bits(run[~fresh]) and bits(start1[~fresh]) == bits(start0[~fresh])
            assert not run1[fresh].any() and np.array_equal(start1, want["start_xy"])
            assert bits(host(self.last)) == bits(last) and bits(host(self.sum)) == bits(total)
            trace.append(tuple(x.tobytes() for x in (run, last, total, run1, start1)) + ((host(self.level).tobytes(),) if self.level is not None else ()))
        return trace


@pytest.mark.parametrize("dtype,v0", ROBOTS)
def test_entries_match_the_restatement_on_the_scenarios(dtype, v0):
    """N = 1, 17 (a tail workgroup of one env) and 33, RANDOM_TOP on with teacher terms and off without.
    Measured (MI355X), both robots: largest relative error 1.1e-16 on the float64 path, 0 on the float32 path (the statistics are
    float64 on either); 54 ups, 30 downs, 18 neither, 15 + 15 graduations, 10 NaN positions, 20 non-finite steps."""
    np_dtype = np.float64 if dtype == "f64" else np.float32
    err, seen = [0.0], {}
    for n in (1, 17, 33):
        for top, teacher in ((True, True), (False, False)):
            sc = er.scenario(n, np_dtype, random_top=top, teacher=teacher, t_episode=T_EPISODE)
            played, count = er.play(sc)
            assert count["in_band"] == 0
            Direct(sc, dtype, v0).play(sc, played, err)
            for k, v in count.items():
                seen[k] = seen.get(k, 0) + v
    print(f"policy episode entries vs numpy, {dtype} v0={v0}: largest relative error {err[0]:.3e}", seen)
    for k in ("up", "down", "neither", "graduate_random", "graduate_top", "level_below", "level_above", "nan_position", "nan_step", "timeout",
              "termination", "never_finishes", "finishes_twice", "teacher_null"):
        assert seen[k] >= 1, k
    assert err[0] <= 1e-12, err[0]


def test_curriculum_off_and_no_level_pointer():
    """the statistics alone: with the curriculum off the levels stay where they are; with no level pointer the LEVEL column is 0"""
    sc = er.scenario(17, t_episode=T_EPISODE)
    err = [0.0]
    d = Direct(sc, "f64", False, curriculum=False)
    d.play(sc, er.play(sc, curriculum=False)[0], err)
    assert np.array_equal(host(d.level), sc["level0"])
    d = Direct(sc, "f64", False, curriculum=False, level=False)
    d.play(sc, er.play(sc, curriculum=False, level=False)[0], err)
    assert not host(d.last)[:, er.LEVEL].any() and err[0] <= 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_split_batch_records_and_draws_what_the_whole_batch_does(dtype):
    """32 envs against two runs of 16 with the terrain's env_offset 0 / 16: every output of every call bit for bit, the random
    levels of the graduates among them"""
    np_dtype = np.float64 if dtype == "f64" else np.float32
    sc = er.scenario(32, np_dtype, random_top=True, t_episode=T_EPISODE)
    played, count = er.play(sc)
    assert count["graduate_random"] >= 4
    err = [0.0]
    whole = Direct(sc, dtype, False).play(sc, played, err)
    for sl in (slice(0, 16), slice(16, 32)):
        part = er.rows_of(sc, sl)
        assert part["curriculum"]["env_offset"] == sl.start
        trace = Direct(part, dtype, False).play(part, er.play(part)[0], err)
        for a, b in zip(trace, whole):
            for x, y in zip(a, b):
                rows = len(y) // 32
                assert x == y[sl.start * rows:sl.stop * rows]
    assert err[0] <= 1e-12


def test_calls_are_rejected_with_a_message():
    from tsid_control_amd import _lib
    sc = er.scenario(4, t_episode=T_EPISODE)
    d = Direct(sc, "f64", False)
    wc = d.wc
    config = lambda p, k=_lib.POL_EPP_NPARAMS: wc._call("tsidb_policy_episode_config", np.asarray(p, dtype=np.float64).ctypes.data_as(vp) if p is not None else None, k)
    for p, msg in (([1, 0.5, 0.5, 1, 0], "TSIDB_POL_EPP_NPARAMS"), ([1, float("nan"), 0.5, 1], "non-finite"), ([2, 0.5, 0.5, 1], "flags"),
                   ([1, 0.5, 0.5, 0.5], "flags"), ([1, 0.0, 0.5, 1], "up_distance must be positive"), ([1, -1.0, 0.5, 1], "up_distance must be positive"),
                   ([0, 0.5, -0.1, 0], "down_fraction must be >= 0")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_config: .*" + msg):
            config(p, len(p))
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_EPP_NPARAMS"):
        config(None, 3)
    config([0, 0.0, 0.5, 0])                                  # (up_distance is not looked at with the curriculum off)
    config([1, sc["curriculum"]["up_distance"], sc["curriculum"]["down_fraction"], 1])
    # nothing of the rejected vectors was taken: the scenario plays as ever
    err = [0.0]
    d.play(sc, er.play(sc)[0], err)
    assert err[0] <= 1e-12
    end = lambda ep=d.ep, qpos=d.qpos.data_ptr(), ld=wc.NROW: wc._call(
        "tsidb_policy_episode_end", C.byref(d.bufs), C.byref(ep) if ep is not None else None, vp(qpos) if qpos else None,
        vp(d.rows.data_ptr()), vp(d.rows.data_ptr()), ld, wc._stream())
    begin = lambda ep=d.ep, ld=wc.NROW, qpos=d.qpos.data_ptr(): wc._call(
        "tsidb_policy_episode_begin", C.byref(d.bufs), C.byref(ep) if ep is not None else None, vp(d.rows.data_ptr()), ld,
        vp(qpos) if qpos else None, wc._stream())
    for bad in (dict(ep=None), dict(ep=_lib.PolicyEpisode(d.run.data_ptr(), None, d.last.data_ptr(), d.sum.data_ptr(), None, None))):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_end: null buffer in tsidb_policy_episode"):
            end(**bad)
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_begin: null buffer in tsidb_policy_episode"):
            begin(**bad)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_end: null buffer or row stride"):
        end(qpos=None)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_end: null buffer or row stride"):
        end(ld=0)
    with pytest.raises(_lib.TsidbError, match="TSIDB_NROW"):
        begin(ld=3)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_episode_begin: null buffer"):
        begin(qpos=None)
    with pytest.raises(_lib.TsidbError, match="null buffer in tsidb_policy_bufs"):
        wc._call("tsidb_policy_episode_end", None, C.byref(d.ep), vp(d.qpos.data_ptr()), vp(d.rows.data_ptr()), vp(d.rows.data_ptr()), 1, wc._stream())
    # the curriculum's own needs: a level pointer, a terrain, an episode length
    no_level = _lib.PolicyEpisode(d.run.data_ptr(), d.start_xy.data_ptr(), d.last.data_ptr(), d.sum.data_ptr(), None, None)
    with pytest.raises(_lib.TsidbError, match="the curriculum needs the level buffer"):
        end(ep=no_level)
    begin(ep=no_level)
    wc._call("tsidb_policy_terrain_config", None, 0)
    with pytest.raises(_lib.TsidbError, match="the curriculum needs a terrain"):
        end()
    ter = d.env.ter_params
    wc._call("tsidb_policy_terrain_config", ter.ctypes.data_as(vp), len(ter))
    base = d.env.params.copy()
    base[_lib.POL_P_MAX_EPISODE_STEPS] = 0
    scale, default = d.env.action_scale, d.env.default_joint_pos
    wc._call("tsidb_policy_config", base.ctypes.data_as(vp), len(base), scale.ctypes.data_as(vp), default.ctypes.data_as(vp), d.env.term_body_mask)
    with pytest.raises(_lib.TsidbError, match="the curriculum needs max_episode_steps > 0"):
        end()
    config([0, 0.0, 0.0, 0])
    end()                                                    # the statistics alone need neither
    config(None, 0)                                          # the slice off again
    for call in (end, begin):
        with pytest.raises(_lib.TsidbError, match="call tsidb_policy_episode_config first"):
            call()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- (b) in the env
ENV = dict(decimation=2, mode="motor", action_scale=1.0, command_range=CMD, max_episode_steps=6, seed=3,
           reward_weights=dict(track_lin_vel=1.0, alive=0.2, action_rate=-0.01, termination=-5.0),
           randomization=dict(seed=7, reset_joint_pos=0.1, reset_xy=0.5, reset_yaw=np.pi),
           terrain=dict(seed=5, friction=(0.4, 1.0), step_height=(0.0, 0.01), num_levels=3, scan_x=(-0.2, 0.2, 3), scan_y=(0.0, 0.0, 1)))
# (a driven robot moves 0.1 .. 2 mm in an episode of 6 x 2 sim steps, and its command asks for 0.5 .. 12 mm: both directions occur)
CUR = dict(up_distance=4e-4, down_fraction=0.5, random_top=True)
STATE = ("qpos", "qvel", "ncon", "con_pairs")


def hand_step(env, action, before_reset=None, after_redraw=None):
    """step() stage by stage (no tsid), with a hook where the episode's last state stands and one where its first does"""
    wc = env.wc
    env._act(action)
    if env._dr_push:
        env._perturb()
    wc.sim_steps(env.decimation)
    env._reward()
    if before_reset:
        before_reset()
    if env._episode is not None:
        env._episode_end()
    wc.reset_done()
    if env._dr_reset:
        env._reset_noise()
    env._terrain_reset()
    if after_redraw:
        after_redraw()
    if env._episode is not None:
        env._episode_begin()
    env._obs()
    env._height_scan()


def reference_of_env(env):
    from tsid_control_amd import _lib
    cur = None
    if env.curriculum is not None:
        c, ter = env.curriculum, env.ter_params
        cur = dict(up_distance=c.up_distance, down_fraction=c.down_fraction, random_top=c.random_top, seed=int(ter[_lib.POL_TER_SEED]),
                   env_offset=int(ter[_lib.POL_TER_ENV_OFFSET]), t_episode=t_episode(env))
    ref = er.PolicyEpisodeReference(env.num_envs, int(env.ter_params[_lib.POL_TER_NUM_LEVELS]), cur)
    ref.begin(np.ones(env.num_envs), host(env.wc.qpos))                # the constructor's reset started episode 1
    return ref


@pytest.mark.parametrize("dtype,v0", ROBOTS)
def test_env_keeps_the_restatements_records_and_levels(dtype, v0):
    """33 envs x 40 steps, motor mode, episodes of at most 6 steps, half of the envs driven hard with NaN-action restarts; the
    restatement runs on the device's own buffers as they stand before the reset.  A twin without the slice, its terrain_level
    written by hand from the restatement before each reset, steps bit-identically; step() itself is the staged loop.
    Measured (MI355X): 213 episodes (30 terminations, 183 timeouts); v1 robot 109 ups, 104 downs, 15 graduations, v0 192 / 21 / 69;
    largest relative error 1.7e-18 (float64), 0 (float32)."""
    n, steps = 33, 40
    env, auto, twin = make_env(n, dtype, v0, curriculum=CUR, **ENV), make_env(n, dtype, v0, curriculum=CUR, **ENV), make_env(n, dtype, v0, **ENV)
    wc = env.wc
    assert env.episode_last.shape == (n, er.NREC) and env.episode_sum.dtype == torch.float64 and twin._episode is None
    ref = reference_of_env(env)
    assert np.array_equal(host(env.episode_start_xy), ref.start_xy) and not host(env.episode_sum).any()
    err, seen = [0.0], dict(episodes=0, terminations=0, timeouts=0, up=0, down=0, graduated=0)
    level = host(env.terrain_level)
    box = {}

    def before_reset():
        torch.cuda.synchronize()
        box["level"] = ref.end(host(env.terms), None, host(env.reward), host(env.done), host(env.timeout), host(env.ep_len), host(env.episode),
                               host(env.command), host(wc.qpos), box["level"])

    for t in range(steps):
        action = driven(n, env.NA, 300 + t, env, step=t)
        box["level"] = level
        hand_step(env, action, before_reset, lambda: (torch.cuda.synchronize(), ref.begin(host(env.done), host(wc.qpos))))
        level = box["level"]
        # the twin: the same stages without the slice, the level of the next episodes written by hand before the reset
        twin._act(action)
        twin.wc.sim_steps(twin.decimation)
        twin._reward()
        twin.terrain_level.copy_(torch.as_tensor(level, device=wc.device))
        twin.wc.reset_done()
        twin._reset_noise()
        twin._terrain_reset()
        twin._obs()
        twin._height_scan()
        auto.step(action)
        torch.cuda.synchronize()
        fresh = host(env.done) != 0
        seen["episodes"] += int(fresh.sum())
        seen["timeouts"] += int((fresh & (host(env.timeout) != 0)).sum())
        seen["terminations"] += int((fresh & (host(env.timeout) == 0)).sum())
        for k in ("up", "down", "graduated"):
            seen[k] += int(ref.moved[k].sum())
        compare(host(env.episode_last), ref.last, err)
        compare(host(env.episode_sum), ref.sum, err)
        err[0] = max(err[0], rel(host(env.episode_run), ref.run))
        assert np.array_equal(host(env.episode_start_xy), ref.start_xy)
        assert np.array_equal(host(env.terrain_level), level)
        for k in STATE + ("env_params", "terrain"):
            assert same(getattr(wc, k), getattr(twin.wc, k)), (t, k)
        for a, b in ((env.obs, twin.obs), (env.reward, twin.reward), (env.done, twin.done), (env.height_scan, twin.height_scan)):
            assert same(a, b), t
        for a, b in zip(env.written(), auto.written()):
            assert same(a, b), t
    print(f"policy episode in the env, {dtype} v0={v0}: largest relative error {err[0]:.3e}", seen, "levels", np.bincount(level, minlength=3).tolist())
    assert seen["terminations"] >= 1 and seen["timeouts"] >= 1 and seen["up"] >= 1 and seen["down"] >= 1, seen
    assert err[0] <= 1e-12, err[0]
    # episode_stats(): the means of the restated records, then sum is cleared
    count, timeouts, mean = ref.means()
    stats = env.episode_stats()
    assert all(v.dim() == 0 and v.dtype == torch.float64 and v.device == wc.device for v in stats.values())
    from tsid_control_amd import _lib
    assert list(stats) == ["episodes", "timeouts", "length", "return", "displacement", "level"] + ["rew_" + k for k in _lib.POL_TERMS]
    assert float(stats["episodes"]) == count == seen["episodes"] and float(stats["timeouts"]) == timeouts == seen["timeouts"]
    got = np.array([float(v) for v in stats.values()][2:])
    assert rel(got, mean[er.LENGTH:er.TEACH]) <= 1e-12
    assert not host(env.episode_sum).any() and float(env.episode_stats()["episodes"]) == 0


def test_statistics_alone_change_nothing_of_the_env():
    """episode_stats = True, no curriculum: sim state, obs, reward, done and every tensor the twin writes bit-identical to a
    twin built without the slice; the levels stay the caller's"""
    n, steps = 33, 20
    env, twin = make_env(n, episode_stats=True, **ENV), make_env(n, **ENV)
    lvl = torch.arange(n, dtype=torch.int32, device=env.device) % 3
    for e in (env, twin):
        e.terrain_level.copy_(lvl)
    episodes = 0
    for t in range(steps):
        action = driven(n, env.NA, 300 + t, env, step=t)
        out, out2 = env.step(action), twin.step(action)
        episodes += int(env.done.sum())
        for a, b in zip(out[:3], out2[:3]):
            assert same(a, b), t
        assert sorted(set(out[3]) - set(out2[3])) == ["episode_last", "episode_sum"]
        theirs = list(twin.written())
        mine = list(env.written())
        assert len(mine) == len(theirs) + 4
        for a, b in zip(mine, theirs):
            assert same(a, b), t
    assert episodes >= 2 * n and torch.equal(env.terrain_level, lvl)
    assert float(env.episode_stats()["episodes"]) == episodes
    last = host(env.episode_last)
    assert set(last[:, er.LEVEL].tolist()) == {0.0, 1.0, 2.0} and (last[:, er.COUNT] == 1).all() and not last[:, er.TEACH:].any()


def test_teacher_terms_are_summed_with_tsid_in_the_loop():
    """tsid = "stand", residual mode: the TEACH columns are the sums of teacher_terms, RETURN the reward with the teacher's share"""
    from test_gpu_policy_tsid import TEACH
    n, steps = 8, 7
    env = make_env(n, conf_of(closed_loop=True), decimation=2, mode="residual", action_scale=0.05, max_episode_steps=3, tsid="stand",
                   teacher_weights=TEACH, episode_stats=True)
    ref = er.PolicyEpisodeReference(n)
    ref.begin(np.ones(n), host(env.wc.qpos))
    for t in range(steps):
        env.step(driven(n, env.NA, 700 + t, env, 0.5))
        torch.cuda.synchronize()
        # (no reset noise, no terrain: the sums need nothing the reset wipes; the displacement does and is left to the test above)
        ref.run[:, er.LENGTH] += 1
        ref.run[:, er.RETURN] += er.finite(host(env.reward))
        ref.run[:, er.TERMS:er.TEACH] += er.finite(host(env.terms))
        ref.run[:, er.TEACH:] += er.finite(host(env.teacher_terms))
        fresh = host(env.done) != 0
        cols = [er.RETURN] + list(range(er.TERMS, er.NREC))
        assert rel(host(env.episode_last)[fresh][:, cols], ref.run[fresh][:, cols]) <= 1e-12
        ref.run[fresh] = 0
    stats = env.episode_stats()
    assert float(stats["episodes"]) >= 2 * n and float(stats["teacher_contact_match"]) > 0 and list(stats)[-4:] == ["teacher_" + k for k in
                                                                                                               ("track_com", "track_feet", "contact_match", "deviation")]


def test_captured_step_replays_the_statistics_bit_identically():
    n, steps = 33, 14
    eager, env = make_env(n, curriculum=CUR, **ENV), make_env(n, curriculum=CUR, **ENV)
    buf = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
    written = list(env.written())
    assert any(x is env.episode_sum for x in written) and any(x is env.terrain_level for x in written)
    g, _ = capture(lambda: env.step(buf), written)
    episodes = 0
    for t in range(steps):
        action = driven(n, env.NA, 300 + t, env, step=t)
        buf.copy_(action)
        g.replay()
        eager.step(action)
        torch.cuda.synchronize()
        episodes += int(env.done.sum())
        for a, b in zip(env.written(), eager.written()):
            assert same(a, b), t
    assert episodes >= 2 * n and float(env.episode_sum[:, er.COUNT].sum()) == episodes


def test_rollout_is_the_hand_driven_loop():
    from test_gpu_policy_actor import small_actor
    n, T = 16, 12
    env, twin = make_env(n, curriculum=CUR, **ENV), make_env(n, curriculum=CUR, **ENV)
    pa, pb = small_actor(env, seed=8)[0], small_actor(twin, seed=8)[0]
    st = env.rollout(pa, T)
    for t in range(T):
        _, reward, done, info = twin.step(pb.act()["action"])
        assert same(st.reward[t], reward) and same(st.done[t], done)
    torch.cuda.synchronize()
    for a, b in zip(env.written(), twin.written()):
        assert same(a, b)
    assert float(env.episode_sum[:, er.COUNT].sum()) == float(st.done.sum()) >= n
