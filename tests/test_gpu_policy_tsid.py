"""TSID in the loop of the policy environment on the GPU (PolicyEnv(tsid=...); tsidb_policy_teacher / _teacher_obs): the two
kernels against the numpy restatement (tests/policy_teacher_reference.py) on the device's own states, the identities that tie
a residual-mode step to the hand-driven closed loop it wraps - standing and walking -, restarts with a replanned walk, graph
capture, the unchanged defaults and the errors.

Gates, those of tests/test_gpu_policy_env.py.  float64: 1e-12 * max(1, |x|) on teacher_terms, teacher_action, reward and
teacher_obs (inputs are O(1e-3 .. 10), sums have at most 20 terms); done, timeout, the termination term and contact_match
exact.  float32: the device against the float64 restatement fed the same float32 states; gate = 2 x the error the restatement
run in np.float32 arithmetic shows against its float64 self on those states (computed in the test, printed)."""
import copy
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_teacher_reference import TeacherReference  # noqa: E402
from policy_testlib import conf_of, host, make_env, rel, replay_against_eager, staged_step  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHTS = dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-1.0, base_height=-10.0,
               action_rate=-0.01, joint_vel=-1e-3, feet_air_time=1.0, alive=0.2, termination=-5.0)
TEACH = dict(track_com=1.5, track_feet=0.75, contact_match=0.25, deviation=-0.02)


def standing_conf(dtype="f64", v0=False):
    return conf_of(dtype, v0, closed_loop=True)


def walking_conf():
    from tsid_control_amd import RobotConfig
    from tsid_control_amd.walk_planner import op3_closed_loop_walking_conf
    return op3_closed_loop_walking_conf(RobotConfig())


def hashed(shape, key, env, scale=1.0):
    """pseudo-random values in +-scale from an integer hash of (key, index): the same on every run, no generator state"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(key) * np.uint64(1000003)
    with np.errstate(over="ignore"):
        x = (i ^ (i >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = (x >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    return torch.as_tensor(((2 * u - 1) * scale).reshape(shape)).to(env.device, env.dtype).contiguous()


def reference_of(env, dtype=np.float64):
    from tsid_control_amd import _lib
    wc = env.wc
    return TeacherReference(np.asarray(wc.model["mj_ctrl_qidx"]), np.asarray(wc.model["mj_geom_body"]),
                            (wc._named_site("lf_imu")[0], wc._named_site("rf_imu")[0]), env.action_scale, env.default_joint_pos,
                            nq=wc.NQ, nv=wc.NV, clip=env.params[_lib.POL_P_CLIP], mode=env.mode,
                            sigma_com=env.teach_params[_lib.POL_TEACH_SIGMA_COM], sigma_foot=env.teach_params[_lib.POL_TEACH_SIGMA_FOOT],
                            weights=dict(zip(_lib.POL_TEACH_TERMS, env.teach_params[_lib.POL_TEACH_WEIGHTS:])),
                            term_weight=env.params[_lib.POL_P_WEIGHTS + 11], dtype=dtype)


# ---------------------------------------------------------------------------- (1) the kernels against the numpy restatement
@pytest.mark.parametrize("mode", ["residual", "motor", "position"])
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_kernels_match_the_numpy_restatement(dtype, v0, mode):
    """12 policy steps of 5 standing envs (a partial last workgroup), decimation 2, hashed actions, delays 0 .. 2, a filter, an
    actuator with scale 0, episodes of 5 steps; the restatement follows the device's own buffers.  Between the reward and the
    teacher launch the test fails TSID's QP by hand (status = 1): at step 2 for env 0 and for env 3, whose base the test has
    dropped below the fall height so that the reward launch has terminated it already; at step 4 for env 1, which has just
    timed out; at step 7 for env 2."""
    n, steps, na = 5, 12, 18 if v0 else 20
    scale = np.full(na, dict(residual=0.05, motor=0.3, position=0.25)[mode])
    scale[4] = 0.0
    env = make_env(n, standing_conf(dtype, v0), tsid="stand", mode=mode, decimation=2, action_scale=scale, action_clip=0.8,
                   default_joint_pos=None if mode == "position" else np.linspace(-0.02, 0.02, na), filter_alpha=0.7,
                   delay=(torch.arange(n, dtype=torch.int32) % 3).to("cuda:0"), max_episode_steps=5, reward_weights=WEIGHTS,
                   teacher_weights=TEACH, sigma_com=0.02, sigma_foot=0.01, seed=5)
    wc = env.wc
    ref = reference_of(env)
    low = reference_of(env, np.float32) if dtype == "f32" else None
    keys = ("teacher_terms", "teacher_action", "reward", "teacher_obs")
    err, base = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    fail_at = {2: [0, 3], 7: [2]}
    seen = dict(failed=0, already_terminated=0, timed_out=0, restarted=0, natural_failures=0)
    for t in range(steps):
        action = hashed((n, na), 100 + t, env, 1.0)
        pre, post = {}, {}

        def drop():
            if t == 2:
                wc.qpos[3, 2] = 0.05

        def fail_and_grab():
            torch.cuda.synchronize()
            seen["natural_failures"] += int((wc.status != 0).sum())
            targets = fail_at.get(t, [])
            if t == 4:    # an env that has just timed out (env 1, unless TSID failed on it before)
                targets = np.flatnonzero(host(env.timeout) == 1)[:1].tolist()
            for e in targets:
                wc.status[e] = 1
            torch.cuda.synchronize()
            pre.update(rows=host(wc.rows), q=host(wc.q), tau=host(wc.tau), status=host(wc.status), ctrl=host(wc.ctrl), ncon=host(wc.ncon),
                       con_pairs=host(wc.con_pairs), com_ref=host(wc.com_ref), foot_ref=host(wc.foot_ref), contact_active=host(wc.contact_active),
                       reward=host(env.reward), done=host(env.done), timeout=host(env.timeout), terms=host(env.terms))

        def grab():
            torch.cuda.synchronize()
            post.update(teacher_terms=host(env.teacher_terms), teacher_action=host(env.teacher_action), reward=host(env.reward),
                        done=host(env.done), timeout=host(env.timeout), terms=host(env.terms), rows=host(wc.rows))

        staged_step(env, action, before_reward=drop, after_reward=fail_and_grab, after_teacher=grab)
        torch.cuda.synchronize()
        want = ref.teacher(**pre)
        # flags exact
        assert np.array_equal(post["done"], want["done"]) and np.array_equal(post["timeout"], want["timeout"]), t
        assert np.array_equal(post["terms"][:, 11], want["terms"][:, 11]) and np.array_equal(post["terms"][:, :11], pre["terms"][:, :11]), t
        assert np.array_equal(post["teacher_terms"][:, 2], want["teacher_terms"][:, 2]), t
        assert np.array_equal(post["rows"][:, :wc.NOBS], pre["rows"][:, :wc.NOBS])            # the tick's row is only read
        failed = pre["status"] != 0
        assert (post["done"][failed] == 1).all() and (post["timeout"][failed] == 0).all() and (post["terms"][failed, 11] == 1).all()
        assert np.array_equal(post["done"][~failed], pre["done"][~failed]) and np.array_equal(post["timeout"][~failed], pre["timeout"][~failed])
        seen["failed"] += int(failed.sum())
        seen["already_terminated"] += int((failed & (pre["terms"][:, 11] == 1)).sum())
        seen["timed_out"] += int((failed & (pre["timeout"] == 1)).sum())
        seen["restarted"] += int(post["done"].sum())
        # the reward without the restatement: the weighted terms, and the termination weight once per episode end
        w = np.array([TEACH[k] for k in ("track_com", "track_feet", "contact_match", "deviation")])
        plain = pre["reward"] + post["teacher_terms"].astype(np.float64) @ w + np.where(failed & (pre["terms"][:, 11] == 0), -5.0, 0.0)
        assert rel(post["reward"], plain) <= (1e-12 if dtype == "f64" else 1e-5), t
        if t == 2:    # env 3 paid the termination weight in the reward launch
            assert pre["terms"][3, 11] == 1 and failed[3] and failed[0]
        after = dict(done=post["done"], rows=host(wc.rows), qpos=host(wc.qpos), tau=host(wc.tau), com_ref=host(wc.com_ref),
                     foot_ref=host(wc.foot_ref), contact_active=host(wc.contact_active))
        obs64 = ref.teacher_obs(**after)
        got_obs = host(env.teacher_obs)
        fresh = post["done"] != 0
        assert not got_obs[fresh, 2:5].any() and not got_obs[fresh, 8:].any()                  # exactly 0 for the restarted envs
        assert np.array_equal(got_obs[:, 0:2], obs64[:, 0:2])
        for k, dev, w64 in (("teacher_terms", post["teacher_terms"], want["teacher_terms"]), ("teacher_action", post["teacher_action"], want["teacher_action"]),
                            ("reward", post["reward"], want["reward"]), ("teacher_obs", got_obs, obs64)):
            err[k] = max(err[k], rel(dev, w64))
        if low is not None:
            w32, o32 = low.teacher(**pre), low.teacher_obs(**after)
            for k, got, w64 in (("teacher_terms", w32["teacher_terms"], want["teacher_terms"]), ("teacher_action", w32["teacher_action"], want["teacher_action"]),
                                ("reward", w32["reward"], want["reward"]), ("teacher_obs", o32, obs64)):
                base[k] = max(base[k], rel(got, w64))
    print(f"teacher kernels vs numpy, {dtype} v0={v0} {mode}: device", {k: f"{v:.3e}" for k, v in err.items()},
          "float32 numpy vs float64 numpy", {k: f"{v:.3e}" for k, v in base.items()}, seen)
    assert seen["failed"] >= 4 and seen["already_terminated"] >= 1 and seen["timed_out"] >= 1 and seen["restarted"] >= 8
    if mode != "residual":
        assert float(env.teacher_action.abs().max()) > 0 and (env.teacher_action[:, 4] == 0).all()
    for k, v in err.items():
        gate = 1e-12 if dtype == "f64" else 2 * base[k]
        assert v <= gate, (k, v, gate)


# ---------------------------------------------------------------------------- (2) residual mode is the hand-driven loop
def test_residual_mode_is_the_hand_driven_closed_loop():
    """16 standing envs, float64, 20 policy steps of 5 closed-loop env steps.  (a) hashed actions through a filter and delays:
    qpos, qvel, tau and the contact lists are those of a second controller with the same ctrl rows registered as a residual and
    stepped by wc.step(decimation).  (b) zero actions, alpha 1, no delay: those of the plain closed loop with no ctrl at all.
    Residuals of at most 0.05 N m: nobody terminates."""
    from tsid_control_amd import WalkController
    n, steps, dec = 16, 20, 5
    conf = standing_conf()
    env = make_env(n, conf, tsid="stand", mode="residual", decimation=dec, action_scale=0.05, filter_alpha=0.6,
                   delay=(torch.arange(n, dtype=torch.int32) % 3).to("cuda:0"), reward_weights=WEIGHTS, teacher_weights=TEACH)
    quiet = make_env(n, conf, tsid="stand", mode="residual", decimation=dec, action_scale=0.05)
    hand, plain = WalkController(copy.copy(conf), num_envs=n, device="cuda:0"), WalkController(copy.copy(conf), num_envs=n, device="cuda:0")
    ctrl = torch.zeros(n, hand.NA, dtype=hand.dtype, device=hand.device)
    hand.set_ctrl(ctrl, "residual")
    zeros = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
    moved = 0.0
    for t in range(steps):
        def grab():
            ctrl.copy_(env.wc.ctrl)

        staged_step(env, hashed((n, env.NA), 300 + t, env, 1.0), after_act=grab)
        moved = max(moved, float(ctrl.abs().max()))
        hand.step(dec)
        obs, reward, done, info = quiet.step(zeros)
        plain.step(dec)
        assert not env.done.any() and not done.any() and not (env.wc.status != 0).any(), t
        for k in ("qpos", "qvel", "tau", "ncon", "con_pairs"):
            assert torch.equal(getattr(env.wc, k), getattr(hand, k)), (t, k)
            assert torch.equal(getattr(quiet.wc, k), getattr(plain, k)), (t, k)
        assert (info["teacher_terms"][:, 3] == 0).all() and (t < 2 or (env.teacher_terms[:, 3] > 0).all())    # (delays of up to 2 steps)
    assert 0.01 < moved <= 0.05 and not torch.equal(env.wc.qpos, quiet.wc.qpos)
    assert (env.episode == 1).all() and (env.ep_len == steps).all() and (quiet.ep_len == steps).all()


# ---------------------------------------------------------------------------- (3) walking
def hand_walker(n, t_start):
    """the hand-driven twin of PolicyEnv(tsid="walk"): controller, device schedule and clock, restarted as the env's reset() does"""
    from tsid_control_amd import WalkController
    from tsid_control_amd.walk_planner import WalkSchedule, op3_walking_posture
    conf = walking_conf()
    conf.sim_enabled = True
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    wc.set_posture_bias(op3_walking_posture())
    clock = torch.zeros(1, dtype=torch.float64, device=wc.device)
    sched = WalkSchedule.on_device(wc, plan=False, foot_press=0.0, t_start=t_start)
    sched.enable_touchdown_feedback(0.6)
    wc.done.fill_(1)
    wc.reset_done()
    sched.plan(wc, done_only=True, new_paths=True, t_device=clock)
    wc.done.zero_()
    return wc, sched, clock


def test_walking_under_a_zero_residual_is_the_hand_driven_walk_and_restarts_replan():
    """16 walkers, float64, t_start = 0.2 s, 150 policy steps of 4 ticks (1.2 s: the start phase, the first step's lift-off and
    touch-down, the second lift-off) under a zero residual: nobody terminates, every env shows single support in teacher_obs,
    and the sim state, tau, contact lists and clock are those of the hand-driven sched.apply / wc.step(1) loop.  Then done is
    forced on three envs: they restart in that step on a new plan at the clock; the others do not notice."""
    n, steps, dec, t_start = 16, 150, 4, 0.2
    env = make_env(n, walking_conf(), tsid="walk", walk=dict(t_start=t_start), mode="residual", decimation=dec, action_scale=0.05,
                   reward_weights=WEIGHTS, teacher_weights=TEACH)
    wc, sched = env.wc, env.sched
    hand, hsched, hclock = hand_walker(n, t_start)
    dt = hand.conf.dt
    zeros = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
    assert (env.episode == 1).all() and (sched.episode == 1).all() and torch.equal(sched.coef, hsched.coef) and torch.equal(sched.com, hsched.com)

    def hand_steps():
        for _ in range(dec):
            hsched.apply(hand, 0.0, t_device=hclock)
            hand.step(1)
            hclock.add_(dt)

    def same(rows=slice(None)):
        for k in ("qpos", "qvel", "tau", "ncon", "con_pairs", "contact_active", "com_ref"):
            assert torch.equal(getattr(wc, k)[rows], getattr(hand, k)[rows]), k
        assert torch.equal(env.clock, hclock)

    single = torch.zeros(n, dtype=torch.bool, device=wc.device)
    lifted, landed = 0, 0
    prev = wc.contact_active.clone()
    for t in range(steps):
        obs, reward, done, info = env.step(zeros)
        hand_steps()
        assert not done.any() and not (wc.status != 0).any(), t
        same()
        act = info["teacher_obs"][:, 0:2]
        assert torch.equal(act, wc.contact_active.to(env.dtype))
        single |= (act == 0).any(1)
        lifted += int(((prev == 1) & (wc.contact_active == 0)).sum())
        landed += int(((prev == 0) & (wc.contact_active == 1)).sum())
        prev = wc.contact_active.clone()
    assert single.all() and lifted >= n and landed >= n
    assert float(env.clock) == pytest.approx(steps * dec * dt, abs=1e-12) and float(wc.qpos[:, 2].min()) > 0.29
    # forced restarts
    ids = torch.tensor([2, 7, 13], device=wc.device)
    others = torch.ones(n, dtype=torch.bool, device=wc.device)
    others[ids] = False
    before = dict(episode=env.episode.clone(), plan_episode=sched.episode.clone(), coef=sched.coef.clone(), t_offset=sched.t_offset.clone(),
                  td=sched.td_latch.clone())

    def force():
        wc.done[ids] = 1

    staged_step(env, zeros, after_teacher=force)
    hand_steps()
    torch.cuda.synchronize()
    assert torch.equal(env.episode[ids], before["episode"][ids] + 1) and torch.equal(sched.episode[ids], before["plan_episode"][ids] + 1)
    assert torch.equal(sched.t_offset[ids], env.clock.to(env.dtype).expand(3)) and (sched.td_latch[ids] == -1).all()
    assert (env.ep_len[ids] == 0).all() and (wc.qvel[ids] == 0).all() and (wc.contact_active[ids] == 1).all()
    tobs = env.teacher_obs
    assert (tobs[ids, 2:5] == 0).all() and (tobs[ids, 8:] == 0).all() and (tobs[ids, 0:2] == 1).all()
    assert not torch.equal(sched.coef[ids], before["coef"][ids])                       # a new path: a new plan
    same(others)
    assert torch.equal(env.episode[others], before["episode"][others]) and torch.equal(sched.coef[others], before["coef"][others])
    assert torch.equal(sched.t_offset[others], before["t_offset"][others]) and (sched.t_offset[others] == 0).all()
    assert (tobs[others, 14:] != 0).any(1).all()
    # and everybody walks on: the restarted envs through their start phase, the others as the hand-driven loop does
    for t in range(25):
        obs, reward, done, info = env.step(zeros)
        hand_steps()
        assert not done.any(), t
    same(others)
    assert (env.ep_len[ids] == 25).all()


# ---------------------------------------------------------------------------- (4) graph capture
def test_captured_walk_step_replays_bit_identically():
    """step() with tsid = "walk", residual mode and every group of the randomisation that tsid allows, captured in a
    torch.cuda.graph on one stream; after the warm-up the state is rewound; 20 replays against 20 eager steps of a twin, bit
    for bit, the device clock included - t_start = 0.1 s puts the first lift-off into policy step 13, and every env times out
    at step 15 (restarts and replans inside the graph)"""
    n, steps = 16, 24
    dr = dict(seed=3, reset_joint_pos=0.02, reset_joint_vel=0.1, reset_base_lin_vel=0.05, reset_base_ang_vel=0.1, noise_ang_vel=0.1,
              noise_gravity=0.02, noise_joint_pos=0.01, noise_joint_vel=0.5, push_interval=6, push_duration=2, push_force_lo=0.1,
              push_force_hi=0.5, command_interval=5, command_zero_prob=0.2)
    kw = dict(tsid="walk", walk=dict(t_start=0.1), mode="residual", decimation=4, action_scale=0.05, filter_alpha=0.8, max_episode_steps=15,
              reward_weights=WEIGHTS, teacher_weights=TEACH, command_range=((0.0, 1.0), (0.0, 0.0), (-1.0, 1.0)),
              delay=(torch.arange(n, dtype=torch.int32) % 4).to("cuda:0"), randomization=dr)
    eager, env = make_env(n, walking_conf(), **kw), make_env(n, walking_conf(), **kw)
    actions = [hashed((n, env.NA), 900 + t, env, 1.0) for t in range(steps)]
    written = list(env.written())
    assert any(x is env.clock for x in written) and any(x is env.sched.coef for x in written) and any(x is env.teacher_obs for x in written)
    restarts = 0
    for t in replay_against_eager(env, eager, actions):
        restarts += int(env.done.sum())
        assert float(env.clock) == pytest.approx((t + 1) * 4 * env.wc.conf.dt, abs=1e-12)
    assert t == steps - 1 and restarts >= n


# ---------------------------------------------------------------------------- (5) the defaults change nothing
def test_defaults_are_the_environment_without_tsid():
    from tsid_control_amd import PolicyEnv, RobotConfig
    n, steps = 16, 15
    kw = dict(num_envs=n, device="cuda:0", decimation=10, action_scale=0.5, filter_alpha=0.7, max_episode_steps=6, reward_weights=WEIGHTS,
              command_range=((0.0, 1.0), (0.0, 0.0), (-1.0, 1.0)), randomization=dict(seed=2, reset_yaw=0.3, reset_xy=0.1, noise_gravity=0.02))
    old, new = PolicyEnv(RobotConfig(), **kw), PolicyEnv(RobotConfig(), tsid=None, walk=None, teacher_weights=None, **kw)
    assert new.tsid is None and new.sched is None and new.clock is None and not hasattr(new, "teacher_obs")
    assert len(list(new.written())) == len(list(old.written()))
    for t in range(steps):
        action = hashed((n, old.NA), 40 + t, old, 0.6)
        o1, r1, d1, i1 = old.step(action)
        o2, r2, d2, i2 = new.step(action)
        assert sorted(i2) == sorted(i1) == ["episode_length", "terms", "timeout"]
        assert torch.equal(old._rows, new._rows) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1["terms"], i2["terms"])
        for k in ("qpos", "qvel", "ncon", "con_pairs", "ctrl"):
            assert torch.equal(getattr(old.wc, k), getattr(new.wc, k)), (t, k)
    assert int(new.episode.sum()) >= 3 * n


# ---------------------------------------------------------------------------- (6) rejections
def test_constructor_rejections_carry_their_message():
    from tsid_control_amd import RobotConfig, _lib
    with pytest.raises(_lib.TsidbError, match="'residual' with tsid"):
        make_env(4, RobotConfig(), mode="residual")
    with pytest.raises(_lib.TsidbError, match="op3_closed_loop_walking_conf"):
        make_env(4, RobotConfig(), tsid="stand")
    with pytest.raises(_lib.TsidbError, match="op3_closed_loop_walking_conf"):
        make_env(4, RobotConfig(), tsid="walk", mode="residual")
    for k, v in (("reset_xy", 0.1), ("reset_yaw", 0.2), ("reset_lift", 0.01)):
        with pytest.raises(_lib.TsidbError, match=k + " cannot be used with tsid"):
            make_env(4, standing_conf(), tsid="stand", randomization={k: v})
    with pytest.raises(_lib.TsidbError, match="unknown teacher terms"):
        make_env(4, standing_conf(), tsid="stand", teacher_weights=dict(track_base=1.0))
    for bad in (0.0, -0.05):
        with pytest.raises(_lib.TsidbError, match="sigma_com and sigma_foot must be positive"):
            make_env(4, standing_conf(), tsid="stand", sigma_com=bad)
    # and what is allowed goes through: joint and velocity reset noise with tsid
    env = make_env(4, standing_conf(), tsid="stand", mode="residual", randomization=dict(reset_joint_pos=0.02, reset_joint_vel=0.1))
    obs, reward, done, info = env.step(torch.zeros(4, env.NA, dtype=env.dtype, device=env.device))
    assert info["teacher_obs"].shape == (4, 14 + env.NA) and not done.any()


def test_entry_points_are_rejected_with_a_message():
    from tsid_control_amd import WalkController, _lib
    n = 4
    wc = WalkController(standing_conf(), num_envs=n, device="cuda:0")
    NA, NOBS = wc.NA, _lib.pol_nobs(wc.NA)
    z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
    t = dict(hist=z(8, n, NA), last=z(n, NA), prev=z(n, NA), cmd=z(n, 3), air=z(n, 2), ep_len=z(n, dt=torch.int32), episode=z(n, dt=torch.int32),
             terms=z(n, 12), timeout=z(n, dt=torch.int32), obs=z(n, NOBS + 4))
    bufs = _lib.PolicyBufs(t["hist"].data_ptr(), t["last"].data_ptr(), t["prev"].data_ptr(), t["cmd"].data_ptr(), t["air"].data_ptr(),
                           t["ep_len"].data_ptr(), t["episode"].data_ptr(), None, t["terms"].data_ptr(), t["timeout"].data_ptr(), t["obs"].data_ptr(), NOBS + 4)
    tt, ta, tobs = z(n, 4), z(n, NA), z(n, 14 + NA)
    vp = C.c_void_p
    p = lambda x: vp(x.data_ptr()) if x is not None else None

    def teacher(rows=wc.rows, ld=wc.NROW, terms=tt):
        wc._call("tsidb_policy_teacher", C.byref(bufs), p(rows), ld, p(wc.q), p(wc.tau), p(wc.status), p(wc.ncon), p(wc.con_pairs), p(terms), p(ta),
                 wc._stream())

    def teacher_obs(out=tobs, ld=14 + NA):
        wc._call("tsidb_policy_teacher_obs", C.byref(bufs), p(wc.rows), wc.NROW, p(wc.qpos), p(wc.tau), p(out), ld, wc._stream())

    for call in (teacher, teacher_obs):
        with pytest.raises(_lib.TsidbError, match="no ctrl buffer registered"):
            call()
    wc.set_ctrl(z(n, NA), "residual")
    for call in (teacher, teacher_obs):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_config first"):
            call()
    pp = np.zeros(_lib.POL_NPARAMS)
    pp[_lib.POL_P_CLIP], pp[_lib.POL_P_ALPHA], pp[_lib.POL_P_SIGMA], pp[_lib.POL_P_DECIMATION] = 1.0, 1.0, 0.25, 4
    scale, default = np.full(NA, 0.25), np.zeros(NA)
    wc._call("tsidb_policy_config", pp.ctypes.data_as(vp), _lib.POL_NPARAMS, scale.ctypes.data_as(vp), default.ctypes.data_as(vp), 1)
    for call in (teacher, teacher_obs):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_config first"):
            call()
    good = np.array([0.05, 0.05, 1.0, 1.0, 0.5, -0.1])
    config = lambda q, k=_lib.POL_TEACH_NPARAMS: wc._call("tsidb_policy_teacher_config", q.ctypes.data_as(vp), k)
    for i, v in ((0, 0.0), (1, -0.01), (0, float("nan")), (3, float("inf"))):
        bad = good.copy()
        bad[i] = v
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_config"):
            config(bad)
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_TEACH_NPARAMS"):
        config(good, _lib.POL_TEACH_NPARAMS - 1)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_config first"):      # nothing of a rejected vector was taken
        teacher()
    config(good)
    with pytest.raises(_lib.TsidbError, match="null buffer"):
        teacher(terms=None)
    with pytest.raises(_lib.TsidbError, match="TSIDB_NROW"):
        teacher(ld=wc.NROW - 1)
    with pytest.raises(_lib.TsidbError, match="null buffer"):
        teacher_obs(out=None)
    with pytest.raises(_lib.TsidbError, match="row stride"):
        teacher_obs(ld=13 + NA)
    # without the reference buffers: a second handle that never saw tsidb_set_refs, configured like the first
    from tsid_control_amd.params import P_COUNT
    L, raw, h2 = wc._L, wc.model.raw, C.c_void_p()
    assert L.tsidb_create(raw, len(raw), wc.params.ctypes.data_as(vp), P_COUNT, n, wc.device.index, 0, C.byref(h2)) == 0
    try:
        assert L.tsidb_set_ctrl(h2, p(wc.ctrl), _lib.CTRL_RESIDUAL) == 0
        assert L.tsidb_policy_config(h2, pp.ctypes.data_as(vp), _lib.POL_NPARAMS, scale.ctypes.data_as(vp), default.ctypes.data_as(vp), 1) == 0
        assert L.tsidb_policy_teacher_config(h2, good.ctypes.data_as(vp), _lib.POL_TEACH_NPARAMS) == 0
        rc = L.tsidb_policy_teacher(h2, C.byref(bufs), p(wc.rows), wc.NROW, p(wc.q), p(wc.tau), p(wc.status), p(wc.ncon), p(wc.con_pairs), p(tt), p(ta),
                                    wc._stream())
        assert rc != 0 and b"tsidb_policy_teacher: reference buffers not registered" in L.tsidb_last_error(h2)
        rc = L.tsidb_policy_teacher_obs(h2, C.byref(bufs), p(wc.rows), wc.NROW, p(wc.qpos), p(wc.tau), p(tobs), 14 + NA, wc._stream())
        assert rc != 0 and b"tsidb_policy_teacher_obs: reference buffers not registered" in L.tsidb_last_error(h2)
    finally:
        L.tsidb_destroy(h2)
    # and good calls go through: a standing robot after one closed-loop step is on its CoM reference, both feet down; the reset
    # leaves the foot references at the identity placement (the foot tasks get theirs from a walking schedule), so track_feet
    # measures the soles' distance from the origin
    wc.step(3)
    wc.reward.zero_()
    wc.done.zero_()
    teacher()
    teacher_obs()
    torch.cuda.synchronize()
    assert (wc.foot_ref[:, :, :3] == 0).all()
    feet = torch.exp(-(wc.frames[:, :, 9:12] ** 2).sum((1, 2)) / 0.05 ** 2)
    cb = wc.contact_bodies()                                              # (floor rows: body1 = -1, body2 = the robot's body)
    down = torch.stack([((cb[:, :, 0] == -1) & (cb[:, :, 1] == wc._named_site(s)[0])).any(1) for s in ("lf_imu", "rf_imu")], dim=1)
    assert (tt[:, 0] > 0.99).all() and torch.allclose(tt[:, 1], feet, rtol=1e-12, atol=0) and (tt[:, 3] == 0).all() and (ta == 0).all()
    assert torch.equal(tt[:, 2], (down == (wc.contact_active != 0)).sum(1).to(wc.dtype))
    assert torch.allclose(wc.reward, (tt * torch.as_tensor(good[2:], device=wc.device)).sum(1), rtol=0, atol=1e-12)
    assert (tobs[:, 0:2] == 1).all() and float(tobs[:, 2:5].abs().max()) < 1e-3 and torch.equal(tobs[:, 14:], wc.ctrl_from_tau(wc.tau))
    wc.set_ctrl(None)
    with pytest.raises(_lib.TsidbError, match="no ctrl buffer registered"):
        teacher()
