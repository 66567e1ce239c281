"""The policy environment on the GPU (PolicyEnv; tsidb_policy_act / _reward / _obs): the three kernels against the numpy
restatement (tests/policy_reference.py) from the device's own sim states, the identities that tie a PolicyEnv step to the
hand-driven set_ctrl / sim_steps / reset_done loop it replaces, the actuation delay, the episode lifecycle, graph capture
and the C-ABI's errors.

Gates.  float64: 1e-12 * max(1, |x|) on obs, terms, reward and ctrl (inputs are O(1 .. 50), sums have at most 20 terms: a few
dozen ulp); done, timeout, ep_len and episode exact.  float32: the device against the float64 reference fed the same float32
states and actions; gate = 2 x the error the reference run in np.float32 arithmetic shows against its float64 self on those
states (computed in the test, printed)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_reference import PolicyReference  # noqa: E402
from policy_testlib import conf_of, host, make_env, rel, replay_against_eager, staged_step  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_WEIGHTS = dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-1.0, base_height=-10.0,
                   torques=-1e-4, action_rate=-0.01, joint_vel=-1e-3, feet_air_time=1.0, alive=0.2, termination=-5.0)


def rand(shape, seed, env, scale=1.0):
    """uniform in +-scale, drawn on the host in float64, in the env's type on its device"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(env.device, env.dtype).contiguous()


def reference_of(env, dtype=np.float64):
    """the numpy restatement configured as `env` is, with the env's current per-env state"""
    from tsid_control_amd import _lib
    from tsid_control_amd.params import P_DONE_HEIGHT, P_DONE_TILT, P_DT
    wc, p = env.wc, env.params
    r = PolicyReference(env.num_envs, np.asarray(wc.model["mj_act_dof"]), np.asarray(wc.model["mj_geom_body"]),
                        (wc._named_site("lf_imu")[0], wc._named_site("rf_imu")[0]), env.action_scale, env.default_joint_pos,
                        clip=p[_lib.POL_P_CLIP], alpha=p[_lib.POL_P_ALPHA], sigma=p[_lib.POL_P_SIGMA], h_target=p[_lib.POL_P_H_TARGET],
                        t_air=p[_lib.POL_P_T_AIR], deadband=p[_lib.POL_P_DEADBAND], max_episode_steps=p[_lib.POL_P_MAX_EPISODE_STEPS],
                        decimation=p[_lib.POL_P_DECIMATION], sim_dt=wc.params[P_DT], seed=p[_lib.POL_P_SEED],
                        cmd_lo=p[_lib.POL_P_CMD_LO:_lib.POL_P_CMD_LO + 3], cmd_hi=p[_lib.POL_P_CMD_HI:_lib.POL_P_CMD_HI + 3],
                        weights=dict(zip(_lib.POL_TERMS, p[_lib.POL_P_WEIGHTS:])), term_body_mask=env.term_body_mask,
                        done_height=wc.params[P_DONE_HEIGHT], done_tilt=wc.params[P_DONE_TILT], position_mode=env.mode == "position",
                        dtype=dtype)
    dt = r.dt
    r.ctrl, r.command, r.air = host(wc.ctrl).astype(dt), host(env.command).astype(dt), host(env.air_time).astype(dt)
    r.hist, r.last, r.prev = host(env.act_hist).astype(dt), host(env.last_action).astype(dt), host(env.prev_action).astype(dt)
    r.ep_len, r.episode = host(env.ep_len), host(env.episode)
    if env.delay is not None:
        r.delay = host(env.delay)
    return r


# ---------------------------------------------------------------------------- (1) the kernels against the numpy reference
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_kernels_match_the_numpy_reference(dtype, v0):
    """60 policy steps of 32 envs under random actions, every term weighted, delays 0 .. 7, a filter, a clip that bites,
    commands redrawn at restarts, episodes of at most 12 steps; the reference follows the device's own qpos, qvel, contact
    lists and info (teacher forcing) and keeps its own environment state.
    Measured (MI355X), largest relative error of obs / terms / reward / ctrl: see the printed line; float32 gates are
    computed from the states of the run."""
    n, steps = 32, 60
    delay = (torch.arange(n, dtype=torch.int32) % 8).to("cuda:0")
    env = make_env(n, dtype, v0, decimation=10, action_scale=0.25, action_clip=0.8, delay=delay, filter_alpha=0.7,
                   command_range=((-0.5, 1.0), (-0.3, 0.3), (-1.0, 1.0)), max_episode_steps=12, reward_weights=ALL_WEIGHTS, seed=11,
                   default_joint_pos=np.linspace(-0.05, 0.05, 18 if v0 else 20))
    wc = env.wc
    assert wc.actuator_force is not None                      # the torques term is weighted: the readout is on
    ref = reference_of(env)                                   # float64, the yardstick
    low = reference_of(env, np.float32) if dtype == "f32" else None
    err = dict(obs=0.0, terms=0.0, reward=0.0, ctrl=0.0)
    base = dict(err)
    seen = dict(done=0, timeout=0, terminated=0, first_contact=0, clipped=0)
    for t in range(steps):
        action = rand((n, wc.NA), 100 + t, env, 1.0)
        a = host(action)
        seen["clipped"] += int((np.abs(a) > 0.8).sum())
        sim = {}

        def grab():
            torch.cuda.synchronize()
            sim.update(qpos=host(wc.qpos), qvel=host(wc.qvel), ncon=host(wc.ncon), con=host(wc.con_pairs), info=host(wc.info),
                       force=host(wc.actuator_force), terms=host(env.terms), reward=host(env.reward), done=host(env.done),
                       timeout=host(env.timeout), air=host(env.air_time))

        got_ctrl = {}
        staged_step(env, action, after_act=lambda: got_ctrl.update(c=host(wc.ctrl)), after_reward=grab)
        torch.cuda.synchronize()
        post = [host(x) for x in (wc.qpos, wc.qvel, wc.ncon, wc.con_pairs)]
        # the yardstick: float64 numpy on the device's states
        c64 = ref.act(a).copy()
        rew64, done64 = ref.reward_stage(sim["qpos"], sim["qvel"], sim["ncon"], sim["con"], sim["info"], sim["force"])
        terms64 = ref.terms.copy()
        assert np.array_equal(sim["done"], done64) and np.array_equal(sim["timeout"], ref.timeout), t
        assert rel(sim["air"], ref.air) <= (1e-12 if dtype == "f64" else 1e-5)
        o64 = ref.obs_stage(sim["done"], *post).copy()
        assert np.array_equal(host(env.ep_len), ref.ep_len) and np.array_equal(host(env.episode), ref.episode), t
        assert rel(host(wc.ctrl), ref.ctrl) <= (1e-12 if dtype == "f64" else 1e-6)      # (restarted rows: the default pose)
        assert rel(host(env.command), ref.command) <= (1e-12 if dtype == "f64" else 1e-6)
        seen["done"] += int(done64.sum())
        seen["timeout"] += int(ref.timeout.sum())
        seen["terminated"] += int(terms64[:, 11].sum())
        seen["first_contact"] += int((terms64[:, 9] != 0).sum())
        for k, dev, want in (("ctrl", got_ctrl["c"], c64), ("terms", sim["terms"], terms64), ("reward", sim["reward"], rew64),
                             ("obs", host(env._rows), o64)):
            err[k] = max(err[k], rel(dev, want))
        if low is not None:   # what float32 arithmetic costs on these states: the same restatement in np.float32
            c32 = low.act(a).copy()
            rew32, _ = low.reward_stage(sim["qpos"], sim["qvel"], sim["ncon"], sim["con"], sim["info"], sim["force"])
            o32 = low.obs_stage(sim["done"], *post)       # (every copy restarts the envs the DEVICE restarted)
            for k, got, want in (("ctrl", c32, c64), ("terms", low.terms, terms64), ("reward", rew32, rew64), ("obs", o32, o64)):
                base[k] = max(base[k], rel(got, want))
    print(f"policy kernels vs numpy, {dtype} v0={v0}: device", {k: f"{v:.3e}" for k, v in err.items()},
          "float32 numpy vs float64 numpy", {k: f"{v:.3e}" for k, v in base.items()}, seen)
    assert seen["timeout"] > 0 and seen["clipped"] > 100 and seen["done"] >= seen["timeout"]
    for k, v in err.items():
        gate = 1e-12 if dtype == "f64" else 2 * base[k]
        assert v <= gate, (k, v, gate)


# ---------------------------------------------------------------------------- (2) the sim state is the hand-driven loop's
def test_sim_state_is_that_of_the_hand_driven_loop():
    """a second controller stepped by hand - set_ctrl, sim_steps(decimation), reset_done - with ctrl copied from the env's
    tensor each step: bit-identical qpos, qvel, ncon and con_pairs"""
    from tsid_control_amd import WalkController
    n, steps = 16, 40
    env = make_env(n, decimation=10, action_scale=0.5, filter_alpha=0.6, delay=(torch.arange(n, dtype=torch.int32) % 3).to("cuda:0"),
                   max_episode_steps=15)
    conf = conf_of()
    conf.reference_quirks = False
    hand = WalkController(conf, num_envs=n, device="cuda:0")
    ctrl = torch.zeros(n, hand.NA, dtype=hand.dtype, device=hand.device)
    hand.set_ctrl(ctrl, "position")
    restarts = 0
    for t in range(steps):
        staged_step(env, rand((n, env.NA), 300 + t, env, 1.0), after_act=lambda: ctrl.copy_(env.wc.ctrl))
        hand.sim_steps(10)
        hand.done.copy_(env.done)
        hand.reset_done()
        restarts += int(env.done.sum())
        for k in ("qpos", "qvel", "ncon", "con_pairs"):
            assert torch.equal(getattr(env.wc, k), getattr(hand, k)), (t, k)
    assert restarts >= n          # (every env timed out at least twice, and was restarted on both sides)


# ---------------------------------------------------------------------------- (3) delay
def test_delay_shifts_ctrl_by_whole_policy_steps():
    """alpha = 1: env e has delay e; at step t its ctrl is what the delay-0 env had at step t - e, bit for bit (the default
    pose before anything is that old).  Every env is fed the same action row; the actions are small: nobody falls."""
    n, steps = 8, 30
    default = np.linspace(-0.04, 0.04, 20)
    env = make_env(n, decimation=4, action_scale=0.25, delay=torch.arange(n, dtype=torch.int32, device="cuda:0"), default_joint_pos=default)
    seq = []
    for t in range(steps):
        row = rand((1, env.NA), 500 + t, env, 0.2)
        staged_step(env, row.expand(n, env.NA).contiguous(), after_act=lambda: seq.append(host(env.wc.ctrl)))
        assert not env.done.any()
    for t in range(steps):
        for d in range(n):
            want = seq[t - d][0] if t >= d else default
            assert np.array_equal(seq[t][d], want), (t, d)
    assert len({s[0].tobytes() for s in seq}) == steps


# ---------------------------------------------------------------------------- (4) lifecycle
def test_fallen_envs_restart_in_the_same_step_and_standing_ones_never_do():
    """v1, float64, position mode about the standing pose, 50 Hz.  Envs 0 .. 31 get zero actions: they stand (checked on the
    CPU oracle: 750 sim steps, min height 0.3316 m, up >= 0.99998, soles only).  Envs 32 .. 63 get uniform +-0.5 rad targets,
    redrawn every policy step: on the CPU oracle 20 of 20 seeds fall within 470 sim steps (torso on the floor, height ~0.1 m).
    100 policy steps here."""
    n, steps, half = 64, 100, 32
    env = make_env(n, decimation=10, action_scale=1.0, reward_weights=dict(alive=1.0, termination=-1.0))
    still = make_env(n, decimation=10, action_scale=1.0, reward_weights=dict(alive=1.0, termination=-1.0))
    wc = env.wc
    q0, default = wc.qpos.clone(), torch.as_tensor(env.default_joint_pos, device=wc.device)
    assert torch.equal(q0[0, 3:7], torch.tensor([1.0, 0, 0, 0], dtype=wc.dtype, device=wc.device))      # a proper wxyz reset
    fell = torch.zeros(n, dtype=torch.bool, device=wc.device)
    zeros = torch.zeros(n, env.NA, dtype=wc.dtype, device=wc.device)
    for t in range(steps):
        action = rand((n, env.NA), 700 + t, env, 0.5)
        action[:half] = 0
        episode = env.episode.clone()
        obs, reward, done, info = env.step(action)
        still.step(zeros)
        d = done != 0
        assert not d[:half].any(), t
        for k in ("qpos", "qvel", "ncon", "con_pairs"):
            assert torch.equal(getattr(wc, k)[:half], getattr(still.wc, k)[:half]), (t, k)
        assert torch.equal(obs[:half], still.obs[:half]) and torch.equal(reward[:half], still.reward[:half])
        fell |= d
        if d.any():
            assert (info["terms"][d, 11] == 1).all() and (info["timeout"][d] == 0).all() and (reward[d] == 0).all()   # alive - termination
            assert torch.equal(wc.qpos[d], q0[d]) and (wc.qvel[d] == 0).all() and (wc.qacc_warmstart[d] == 0).all()
            assert (env.act_hist[:, d] == 0).all() and (env.last_action[d] == 0).all() and (env.prev_action[d] == 0).all()
            assert (env.air_time[d] == 0).all() and (env.ep_len[d] == 0).all()
            assert torch.equal(env.episode[d], episode[d] + 1) and torch.equal(wc.ctrl[d], default.expand(n, -1)[d])
            assert (obs[d, 9 + 3 * env.NA:] == 1).all() and torch.equal(env.priv[d, 3], q0[d, 2])
        assert torch.equal(env.episode[~d], episode[~d]) and (reward[~d] == 1).all()
    assert fell[half:].all(), fell.nonzero().reshape(-1).tolist()
    assert float(wc.qpos[:half, 2].min()) > 0.33 and (env.ep_len[:half] == steps).all() and (env.episode[:half] == 1).all()


def test_every_env_times_out_at_max_episode_steps():
    n = 8
    env = make_env(n, decimation=10, max_episode_steps=5, reward_weights=dict(termination=1.0))
    zeros = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
    for t in range(1, 11):
        obs, reward, done, info = env.step(zeros)
        last = t % 5 == 0
        assert (done == (1 if last else 0)).all() and (info["timeout"] == (1 if last else 0)).all(), t
        assert (info["terms"][:, 11] == 0).all() and (reward == 0).all()
        assert (info["episode_length"] == t % 5).all() and (env.episode == 1 + t // 5).all()


# ---------------------------------------------------------------------------- (5) no host round trip: graph capture
def test_captured_step_replays_bit_identically():
    """step() captured in a torch.cuda.graph on one stream; after the warm-up the state is rewound; 20 replays against 20
    eager steps of a twin, bit for bit - envs time out at step 7 and 14 (restarts inside the graph), half are driven hard"""
    n, steps = 32, 20
    kw = dict(decimation=10, action_scale=1.0, filter_alpha=0.8, max_episode_steps=7, reward_weights=ALL_WEIGHTS,
              command_range=((0.0, 1.0), (0.0, 0.0), (-1.0, 1.0)), delay=(torch.arange(n, dtype=torch.int32) % 4).to("cuda:0"))
    eager, env = make_env(n, **kw), make_env(n, **kw)
    actions = [rand((n, env.NA), 900 + t, env, 0.5) for t in range(steps)]
    for a in actions:
        a[: n // 2] *= 0.1
    restarts = 0
    for t in replay_against_eager(env, eager, actions):
        restarts += int(env.done.sum())
    assert t == steps - 1 and restarts >= 2 * n


# ---------------------------------------------------------------------------- (6) a group that is off launches nothing
def test_launches_of_a_group_that_is_off_return_without_launching():
    """no randomisation, no terrain: tsidb_policy_perturb (before it looks for an xfrc buffer), tsidb_policy_reset_noise and
    tsidb_policy_height_scan return 0 (wc._call raises on anything else) and leave every written tensor as it was, bit for
    bit - with every env flagged done, so that a launch would have had work"""
    n = 4
    env = make_env(n)
    wc, vp = env.wc, C.c_void_p
    assert wc.xfrc is None and env.terrain is None
    wc.done.fill_(1)
    scan = torch.full((n, 4), -7.0, dtype=wc.dtype, device=wc.device)
    torch.cuda.synchronize()
    saved = [x.clone() for x in env.written()]
    wc._call("tsidb_policy_perturb", C.byref(env._bufs), wc._stream())
    wc._call("tsidb_policy_reset_noise", C.byref(env._bufs), vp(wc.rows.data_ptr()), wc.NROW, vp(wc.qpos.data_ptr()), vp(wc.qvel.data_ptr()),
             wc._stream())
    wc._call("tsidb_policy_height_scan", C.byref(env._bufs), vp(wc.qpos.data_ptr()), vp(scan.data_ptr()), 4, wc._stream())
    torch.cuda.synchronize()
    for x, s in zip(env.written(), saved):
        assert torch.equal(x, s)
    assert (scan == -7.0).all()


# ---------------------------------------------------------------------------- (7) errors
def test_calls_are_rejected_with_a_message():
    from tsid_control_amd import WalkController, _lib
    n = 4
    conf = conf_of()
    conf.reference_quirks = False
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    NA, NOBS = wc.NA, _lib.pol_nobs(wc.NA)
    z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
    t = dict(hist=z(8, n, NA), last=z(n, NA), prev=z(n, NA), cmd=z(n, 3), air=z(n, 2), ep_len=z(n, dt=torch.int32), episode=z(n, dt=torch.int32),
             terms=z(n, 12), timeout=z(n, dt=torch.int32), obs=z(n, NOBS + 4))

    def bufs(obs_ld=NOBS + 4, **over):
        p = {k: v.data_ptr() for k, v in t.items()}
        p.update(over)
        return _lib.PolicyBufs(p["hist"], p["last"], p["prev"], p["cmd"], p["air"], p["ep_len"], p["episode"], None, p["terms"], p["timeout"],
                               p["obs"], obs_ld)

    action, vp = z(n, NA), C.c_void_p
    act = lambda b: wc._call("tsidb_policy_act", C.byref(b), vp(action.data_ptr()), wc._stream())
    rew = lambda b: wc._call("tsidb_policy_reward", C.byref(b), vp(wc.qpos.data_ptr()), vp(wc.qvel.data_ptr()), vp(wc.ncon.data_ptr()),
                             vp(wc.con_pairs.data_ptr()), vp(wc.info.data_ptr()), vp(wc.reward.data_ptr()), vp(wc.done.data_ptr()), wc.NROW, wc._stream())
    obs = lambda b: wc._call("tsidb_policy_obs", C.byref(b), vp(wc.rows.data_ptr()), wc.NROW, vp(wc.qpos.data_ptr()), vp(wc.qvel.data_ptr()),
                             vp(wc.ncon.data_ptr()), vp(wc.con_pairs.data_ptr()), wc._stream())
    p = np.zeros(_lib.POL_NPARAMS)
    p[_lib.POL_P_CLIP], p[_lib.POL_P_ALPHA], p[_lib.POL_P_SIGMA], p[_lib.POL_P_DECIMATION] = 1.0, 1.0, 0.25, 10
    scale, default = np.full(NA, 0.25), np.zeros(NA)
    config = lambda pp=p, n_p=_lib.POL_NPARAMS, s=scale, d=default, mask=1: wc._call(
        "tsidb_policy_config", pp.ctypes.data_as(vp), n_p, s.ctypes.data_as(vp), d.ctypes.data_as(vp), mask)
    # no ctrl buffer registered
    for call in (act, rew, obs):
        with pytest.raises(_lib.TsidbError, match="no ctrl buffer registered"):
            call(bufs())
    wc.set_ctrl(z(n, NA), "position")
    # before tsidb_policy_config
    for call in (act, rew, obs):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_config first"):
            call(bufs())
    # bad configurations: nothing of them is taken
    def changed(i, v):
        q = p.copy()
        q[i] = v
        return q
    bad = [dict(pp=changed(_lib.POL_P_ALPHA, 0.0)), dict(pp=changed(_lib.POL_P_ALPHA, 1.5)), dict(pp=changed(_lib.POL_P_ALPHA, -0.1)),
           dict(pp=changed(_lib.POL_P_SIGMA, float("nan"))), dict(pp=changed(_lib.POL_P_WEIGHTS + 3, float("inf"))),
           dict(pp=changed(_lib.POL_P_CLIP, -1.0)), dict(pp=changed(_lib.POL_P_DECIMATION, 0)), dict(n_p=_lib.POL_NPARAMS - 1),
           dict(s=np.full(NA, np.nan)), dict(d=np.full(NA, np.inf)), dict(mask=1 << wc.NB), dict(pp=changed(_lib.POL_P_CMD_LO, 1.0))]
    for kw in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_config"):
            config(**kw)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_config first"):
        act(bufs())
    config()
    with pytest.raises(_lib.TsidbError, match="null buffer"):
        act(bufs(terms=None))
    with pytest.raises(_lib.TsidbError, match="obs row stride"):
        obs(bufs(obs_ld=NOBS))
    with pytest.raises(_lib.TsidbError, match="null action"):
        wc._call("tsidb_policy_act", C.byref(bufs()), None, wc._stream())
    # and a good call goes through: the observation of the reset state
    wc.done.fill_(1)
    obs(bufs())
    torch.cuda.synchronize()
    assert torch.equal(t["obs"][:, 3:6], torch.tensor([0.0, 0.0, -1.0], dtype=wc.dtype, device=wc.device).expand(n, 3))
    assert (t["episode"] == 1).all() and (t["obs"][:, NOBS - 2:NOBS] == 1).all() and torch.equal(t["obs"][:, NOBS + 3], wc.qpos[:, 2])
    # unregistering ctrl closes the door again
    wc.set_ctrl(None)
    with pytest.raises(_lib.TsidbError, match="no ctrl buffer registered"):
        act(bufs())
