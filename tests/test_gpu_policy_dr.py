"""The policy randomisation on the GPU (PolicyEnv(randomization=...); tsidb_policy_perturb / _reset_noise and the randomised
tsidb_policy_obs): the kernels against the numpy restatement (tests/policy_dr_reference.py) from the device's own states, off
is off, pushes are the xfrc feature, reproducible and splittable draws, graph replay, and the lifecycle under reset noise.

Gates.  float64: 1e-12 * max(1, |x|) on obs, the state right after the reset noise, the torso force and the commands (a draw is
exact; around it are a product-then-add that may contract to an FMA, a cos / sin and a norm: a few ulp); which steps are
pushed, which envs are resampled or zeroed, ep_len, episode and the flags exact.  float32: the device against the float64
restatement fed the same float32 states; gate = 2 x the error the restatement run in np.float32 shows against its float64
self on those states (computed in the test, printed)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_dr_reference import PolicyDRReference  # noqa: E402
from policy_testlib import conf_of, host, make_env, rel, replay_against_eager, same  # noqa: E402
from test_gpu_policy_env import ALL_WEIGHTS, rand  # noqa: E402

pytestmark = pytest.mark.gpu

# everything on; small intervals so that restarts, resamples and pushes all occur many times in 60 steps
DR = dict(seed=7, reset_joint_pos=0.1, reset_joint_vel=0.5, reset_base_lin_vel=(0.2, 0.1, 0.05), reset_base_ang_vel=0.5, reset_yaw=np.pi,
          reset_xy=0.5, reset_lift=0.01, noise_ang_vel=0.2, noise_gravity=0.05, noise_joint_pos=0.01, noise_joint_vel=1.5,
          push_interval=7, push_duration=2, push_force_lo=0.2, push_force_hi=1.0, command_interval=5, command_zero_prob=0.2)
CMD = ((-0.5, 1.0), (-0.3, 0.3), (-1.0, 1.0))


def dr_reference_of(env, dr, dtype=np.float64):
    """the numpy restatement configured as `env` is, with the env's current per-env state"""
    from tsid_control_amd import _lib
    from tsid_control_amd.params import P_DONE_HEIGHT, P_DONE_TILT, P_DT
    wc, p = env.wc, env.params
    r = PolicyDRReference(env.num_envs, np.asarray(wc.model["mj_act_dof"]), np.asarray(wc.model["mj_geom_body"]),
                          (wc._named_site("lf_imu")[0], wc._named_site("rf_imu")[0]), env.action_scale, env.default_joint_pos,
                          clip=p[_lib.POL_P_CLIP], alpha=p[_lib.POL_P_ALPHA], sigma=p[_lib.POL_P_SIGMA], h_target=p[_lib.POL_P_H_TARGET],
                          t_air=p[_lib.POL_P_T_AIR], deadband=p[_lib.POL_P_DEADBAND], max_episode_steps=p[_lib.POL_P_MAX_EPISODE_STEPS],
                          decimation=p[_lib.POL_P_DECIMATION], sim_dt=wc.params[P_DT], seed=p[_lib.POL_P_SEED],
                          cmd_lo=p[_lib.POL_P_CMD_LO:_lib.POL_P_CMD_LO + 3], cmd_hi=p[_lib.POL_P_CMD_HI:_lib.POL_P_CMD_HI + 3],
                          weights=dict(zip(_lib.POL_TERMS, p[_lib.POL_P_WEIGHTS:])), term_body_mask=env.term_body_mask,
                          done_height=wc.params[P_DONE_HEIGHT], done_tilt=wc.params[P_DONE_TILT], position_mode=env.mode == "position",
                          dtype=dtype, dr=dr)
    dt = r.dt
    r.ctrl, r.command, r.air = host(wc.ctrl).astype(dt), host(env.command).astype(dt), host(env.air_time).astype(dt)
    r.hist, r.last, r.prev = host(env.act_hist).astype(dt), host(env.last_action).astype(dt), host(env.prev_action).astype(dt)
    r.ep_len, r.episode = host(env.ep_len), host(env.episode)
    return r


def driven(n, na, seed, env, hard=1.0, soft=0.05, step=None):
    """actions: the first half of the envs small, the second half large; with `step`, an env of the second half gets a NaN
    action every 23rd (step, env) pair - the sim skips it and the reward stage terminates it: restarts at every episode length,
    not at the timeout alone (the episodes here are too short for a driven robot to reach the floor)"""
    a = rand((n, na), seed, env, hard)
    a[: n // 2] *= soft / hard
    if step is not None:
        e = torch.arange(n, device=a.device)
        a[(e >= n // 2) & ((7 * step + e) % 23 == 0), 0] = float("nan")
    return a.contiguous()


# ---------------------------------------------------------------------------- (1) the kernels against the restatement
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_kernels_match_the_numpy_restatement(dtype, v0):
    """32 envs x 60 policy steps, everything on, episodes of at most 11 steps, half of the envs driven hard; the restatement
    follows the device's own qpos, qvel, contact lists and info and keeps its own environment state.
    Measured (MI355X), 192 restarts (42 terminations), 334 resamples, 114 zeroings, 263 pushes.  float64, largest relative error:
    obs 8.3e-16 (v0 1.7e-16), qpos 1.1e-16, qvel 0, xfrc 1.7e-16, command 1.1e-16.  float32: obs 3.4e-7 against 3.1e-7 of the
    np.float32 restatement (v0 1.2e-7 / 1.2e-7), qpos 6.8e-8 / 5.3e-8, qvel 1.5e-8, xfrc 3.0e-8 and command 3.0e-8 equal to the
    restatement's; the float32 gates are computed from the states of the run."""
    n, steps = 32, 60
    env = make_env(n, dtype, v0, decimation=4, action_scale=1.0, command_range=CMD, max_episode_steps=11, seed=11, randomization=DR,
                   reward_weights=dict(track_lin_vel=1.0, alive=0.2, termination=-5.0))
    wc = env.wc
    assert wc.xfrc is not None and env._dr_push and env._dr_reset
    torch.cuda.synchronize()
    # the first reset drew episode 1: every env its own state, already
    assert len({row.tobytes() for row in host(wc.qpos)}) == n
    ref = dr_reference_of(env, DR)
    low = dr_reference_of(env, DR, np.float32) if dtype == "f32" else None
    err = dict(obs=0.0, qpos=0.0, qvel=0.0, xfrc=0.0, command=0.0)
    base = dict(err)
    seen = dict(done=0, terminated=0, resampled=0, zeroed=0, pushed=0, pushes=0)
    was_active = np.zeros(n, bool)
    for t in range(steps):
        action = driven(n, wc.NA, 100 + t, env, step=t)
        a = host(action)
        env._act(action)
        env._perturb()
        torch.cuda.synchronize()
        xf = host(wc.xfrc)
        f64, active = ref.perturb()
        assert np.array_equal((xf[:, 0, :3] != 0).any(1), active), t                 # which envs are pushed: exact
        assert (xf[:, 0, 2] == 0).all() and (xf[:, 0, 3:] == 0).all() and (xf[:, 1:] == 0).all()
        err["xfrc"] = max(err["xfrc"], rel(xf[:, 0, :3], f64))
        seen["pushed"] += int(active.sum())
        seen["pushes"] += int((active & ~was_active).sum())
        was_active = active
        ref.act(a)
        wc.sim_steps(env.decimation)
        env._reward()
        torch.cuda.synchronize()
        sim = [host(x) for x in (wc.qpos, wc.qvel, wc.ncon, wc.con_pairs, wc.info)]
        done = host(env.done)
        _, done64 = ref.reward_stage(*sim)
        assert np.array_equal(done, done64) and np.array_equal(host(env.timeout), ref.timeout), t
        seen["done"] += int(done.sum())
        seen["terminated"] += int(ref.terms[:, 11].sum())
        wc.reset_done()
        torch.cuda.synchronize()
        pre = host(wc.qpos), host(wc.qvel)
        env._reset_noise()
        torch.cuda.synchronize()
        post = [host(x) for x in (wc.qpos, wc.qvel, wc.ncon, wc.con_pairs)]
        qp64, qv64 = ref.reset_noise(done, *pre)
        fresh = done != 0
        assert np.array_equal(post[0][~fresh], pre[0][~fresh]) and np.array_equal(post[1][~fresh], pre[1][~fresh])   # others: untouched
        err["qpos"], err["qvel"] = max(err["qpos"], rel(post[0], qp64)), max(err["qvel"], rel(post[1], qv64))
        prev_cmd = host(env.command)
        env._obs()
        torch.cuda.synchronize()
        o64 = ref.obs_stage(done, *post).copy()
        cmd = host(env.command)
        assert np.array_equal(host(env.ep_len), ref.ep_len) and np.array_equal(host(env.episode), ref.episode), t
        assert np.array_equal((cmd == 0).all(1), (ref.command == 0).all(1)), t                   # which envs are zeroed: exact
        assert np.array_equal((cmd != prev_cmd).any(1) | ref.zeroed, ref.resampled | fresh), t    # which are resampled: exact
        seen["resampled"] += int(ref.resampled.sum())
        seen["zeroed"] += int(ref.zeroed.sum())
        err["obs"], err["command"] = max(err["obs"], rel(host(env._rows), o64)), max(err["command"], rel(cmd, ref.command))
        assert np.array_equal(host(wc.qpos), post[0]) and np.array_equal(host(wc.qvel), post[1])   # obs noise never touches the state
        if low is not None:   # what float32 arithmetic costs on these states: the same restatement in np.float32
            f32, _ = low.perturb()
            low.act(a)
            low.reward_stage(*sim)
            qp32, qv32 = low.reset_noise(done, *pre)      # (every copy restarts the envs the DEVICE restarted)
            o32 = low.obs_stage(done, *post)
            for k, got, want in (("xfrc", f32, f64), ("qpos", qp32, qp64), ("qvel", qv32, qv64), ("obs", o32, o64), ("command", low.command, ref.command)):
                base[k] = max(base[k], rel(got, want))
    print(f"policy randomisation vs numpy, {dtype} v0={v0}: device", {k: f"{v:.3e}" for k, v in err.items()},
          "float32 numpy vs float64 numpy", {k: f"{v:.3e}" for k, v in base.items()}, seen)
    assert seen["done"] >= 4 * n and seen["terminated"] >= 20 and seen["resampled"] >= n and seen["zeroed"] >= 10 and seen["pushes"] >= 4 * n
    for k, v in err.items():
        gate = 1e-12 if dtype == "f64" else 2 * base[k]
        assert v <= gate, (k, v, gate)


# ---------------------------------------------------------------------------- (2) off is off
def test_zero_randomisation_is_no_randomisation():
    """randomization=None against a randomisation with every value 0: bit-identical over 40 steps with terminations (NaN
    actions: skipped sim steps) and timeouts, each followed by a restart"""
    n, steps = 32, 40
    kw = dict(decimation=5, action_scale=1.0, filter_alpha=0.8, command_range=CMD, max_episode_steps=15, reward_weights=ALL_WEIGHTS, seed=3)
    plain, zero = make_env(n, **kw), make_env(n, randomization={k: 0 for k in DR}, **kw)
    assert zero.randomization is not None and not zero._dr_push and not zero._dr_reset and zero.wc.xfrc is None
    restarts = ended = 0
    for t in range(steps):
        action = driven(n, plain.NA, 200 + t, plain, step=t)
        out_a, out_b = plain.step(action), zero.step(action)
        assert sorted(out_b[3]) == ["episode_length", "terms", "timeout"]
        restarts += int(plain.done.sum())
        ended += int(plain.terms[:, 11].sum())
        for a, b in zip(out_a[:3], out_b[:3]):
            assert same(a, b), t
        for k in ("qpos", "qvel", "ctrl"):
            assert same(getattr(plain.wc, k), getattr(zero.wc, k)), (t, k)
        assert torch.equal(plain.command, zero.command) and torch.equal(plain.episode, zero.episode)
    assert restarts >= 2 * n and ended >= 10          # timeouts and terminations


# ---------------------------------------------------------------------------- (3) pushes are the xfrc feature
def test_pushed_sim_state_is_that_of_the_hand_driven_loop():
    """a second controller stepped by hand - set_ctrl, set_xfrc, sim_steps(decimation), reset_done - with the env's ctrl and
    xfrc copied in each step: bit-identical qpos, qvel, ncon and con_pairs.  Forces of at most 1 N; identity is asserted, not
    survival (how the position-servo robot takes a push has not been measured)."""
    from tsid_control_amd import WalkController
    n, steps = 16, 40
    dr = dict(seed=5, push_interval=6, push_duration=2, push_force_lo=0.2, push_force_hi=1.0, noise_joint_vel=0.5, command_interval=4)
    env = make_env(n, decimation=5, action_scale=0.5, filter_alpha=0.6, max_episode_steps=15, command_range=CMD, randomization=dr)
    conf = conf_of()
    conf.reference_quirks = False
    hand = WalkController(conf, num_envs=n, device="cuda:0")
    ctrl = torch.zeros(n, hand.NA, dtype=hand.dtype, device=hand.device)
    xfrc = torch.zeros(n, hand.NB, 6, dtype=hand.dtype, device=hand.device)
    hand.set_ctrl(ctrl, "position")
    hand.set_xfrc(xfrc)
    restarts = pushed = 0
    for t in range(steps):
        env._act(rand((n, env.NA), 300 + t, env, 1.0))
        env._perturb()
        ctrl.copy_(env.wc.ctrl)
        xfrc.copy_(env.wc.xfrc)
        pushed += int((xfrc[:, 0, :3] != 0).any(1).sum())
        assert float(xfrc.abs().max()) <= 1.0 and (xfrc[:, 1:] == 0).all() and (xfrc[:, 0, 2:] == 0).all()
        env.wc.sim_steps(env.decimation)
        env._reward()
        env.wc.reset_done()
        env._obs()
        hand.sim_steps(5)
        hand.done.copy_(env.done)
        hand.reset_done()
        restarts += int(env.done.sum())
        for k in ("qpos", "qvel", "ncon", "con_pairs"):
            assert torch.equal(getattr(env.wc, k), getattr(hand, k)), (t, k)
    assert restarts >= n and pushed >= 8 * n


# ---------------------------------------------------------------------------- (4) reproducible and splittable
def test_draws_are_reproducible_and_a_split_batch_draws_what_the_whole_batch_draws():
    n, steps = 32, 30
    kw = dict(decimation=4, action_scale=1.0, command_range=CMD, max_episode_steps=9, reward_weights=ALL_WEIGHTS, seed=13)
    whole, twin = make_env(n, randomization=DR, **kw), make_env(n, randomization=DR, **kw)
    halves = [make_env(n // 2, randomization=dict(DR, env_offset=off), **kw) for off in (0, n // 2)]
    other = make_env(n, randomization=dict(DR, seed=DR["seed"] + 1), **kw)
    assert not torch.equal(whole.wc.qpos, other.wc.qpos) and not torch.equal(whole.obs, other.obs)   # a different seed, different draws
    both = (whole.command != 0).any(1) & (other.command != 0).any(1)          # (zeroing draws from the randomisation's seed,
    assert int(both.sum()) > n // 2 and torch.equal(whole.command[both], other.command[both])   # the components from the env's)

    def rows(t, sl):
        """the envs sl of a tensor written(): env-major, but for the action ring [8, N, NA]"""
        return t[:, sl] if t.dim() == 3 and t.shape[0] == 8 and t.shape[1] != 8 else t[sl]

    restarts = 0
    for t in range(steps):
        action = driven(n, whole.NA, 400 + t, whole, step=t)
        whole.step(action)
        twin.step(action)
        for h, sl in zip(halves, (slice(0, n // 2), slice(n // 2, n))):
            h.step(action[sl].contiguous())
        torch.cuda.synchronize()
        restarts += int(whole.done.sum())
        for a, b in zip(whole.written(), twin.written()):
            assert same(a, b), t
        for h, sl in zip(halves, (slice(0, n // 2), slice(n // 2, n))):
            for a, b in zip(whole.written(), h.written()):
                assert same(rows(a, sl), b), (t, sl, tuple(a.shape))
    assert restarts >= 2 * n
    assert len(list(whole.written())) == len(list(halves[0].written())) and any(x is whole.wc.xfrc for x in whole.written())


# ---------------------------------------------------------------------------- (5) graph replay
def test_captured_randomised_step_replays_bit_identically():
    """step() with everything on captured in a torch.cuda.graph on one stream; after the warm-up the state is rewound; 20
    replays against 20 eager steps of a twin, bit for bit - restarts (timeouts at 7 and 14), resamples and pushes inside the
    graph, every draw recomputed from the counters the replayed kernels read"""
    n, steps = 32, 20
    kw = dict(decimation=5, action_scale=1.0, filter_alpha=0.8, max_episode_steps=7, reward_weights=ALL_WEIGHTS, command_range=CMD,
              randomization=DR)
    eager, env = make_env(n, **kw), make_env(n, **kw)
    actions = [driven(n, env.NA, 900 + t, env, 0.5, step=t) for t in range(steps)]
    assert any(x is env.wc.xfrc for x in env.written())
    restarts = pushed = 0
    for t in replay_against_eager(env, eager, actions):
        restarts += int(env.done.sum())
        pushed += int((env.wc.xfrc[:, 0, :3] != 0).any(1).sum())
    assert t == steps - 1 and restarts >= 2 * n and pushed >= 2 * n


# ---------------------------------------------------------------------------- (6) lifecycle
def test_randomised_resets_stand_and_differ():
    """v1, float64, position mode about the standing pose, zero actions, decimation 5, 50 policy steps = 250 sim steps, reset noise
    only.  Checked on the CPU oracle first (oracle.sim_step, ctrl = the default pose, 250 sim steps, the restatement's own draws of
    seed 17 for the 32 envs): episode 1 and episode 2 of all 32 envs stand - figures in DESIGN.md section 4, Policy randomisation."""
    n, steps, again = 32, 50, [3, 9, 20]
    dr = dict(seed=17, reset_joint_pos=0.1, reset_joint_vel=0.5, reset_base_lin_vel=0.2, reset_base_ang_vel=0.5, reset_yaw=np.pi, reset_lift=0.01)
    env = make_env(n, decimation=5, action_scale=0.25, reward_weights=dict(alive=1.0, termination=-1.0), randomization=dr)
    wc = env.wc
    assert wc.xfrc is None and (env.episode == 1).all()      # (no pushes asked: no wrench buffer; the constructor's reset drew episode 1)
    first = wc.qpos.clone()
    assert len({row.tobytes() for row in host(first)}) == n and len({row.tobytes() for row in host(wc.qvel)}) == n
    assert (first[:, 2] == first[0, 2]).all() and (first[:, :2] == 0).all()          # lift is not random, no xy noise asked
    assert float((first[:, 3:7].norm(dim=1) - 1).abs().max()) <= 4 * np.finfo(np.float64).eps and (first[:, 4:6] == 0).all()   # a yaw, nothing else
    assert float(first[:, 7:].abs().max()) <= 0.1 and float(wc.qvel[:, 6:].abs().max()) <= 0.5
    assert torch.equal(env.obs[:, 9:9 + env.NA], first[:, torch.as_tensor(np.asarray(wc.model["mj_act_dof"]) + 1, device=wc.device)]
                       - torch.as_tensor(env.default_joint_pos, device=wc.device))    # the observation is of the randomised state
    zeros = torch.zeros(n, env.NA, dtype=wc.dtype, device=wc.device)
    for t in range(steps):
        if t == 20:
            episode = env.episode.clone()
            env.reset(again)
            assert torch.equal(env.episode[again], episode[again] + 1) and (env.ep_len[again] == 0).all()
            assert (wc.qpos[again] != first[again]).any(1).all()                      # a new episode, a new state
            keep = [e for e in range(n) if e not in again]
            assert torch.equal(env.episode[keep], episode[keep])
        obs, reward, done, info = env.step(zeros)
        assert not done.any(), (t, done.nonzero().reshape(-1).tolist())
    up = 1 - 2 * (wc.qpos[:, 4] ** 2 + wc.qpos[:, 5] ** 2)
    print("randomised resets: final min height", float(wc.qpos[:, 2].min()), "min up", float(up.min()))
    assert (env.episode[again] == 2).all() and (env.ep_len[again] == steps - 20).all() and int(env.episode.sum()) == n + len(again)


# ---------------------------------------------------------------------------- (7) errors
def test_calls_are_rejected_with_a_message():
    """the library's own checks (PolicyRandomization checks the same on the host first): a rejected vector changes nothing,
    a push without a wrench buffer fails, NULL / 0 switches everything off again"""
    import ctypes as C
    from tsid_control_amd import _lib
    n = 4
    env, plain = make_env(n, decimation=4, command_range=CMD, seed=2), make_env(n, decimation=4, command_range=CMD, seed=2)
    wc, vp = env.wc, C.c_void_p
    randomize = lambda p, k=_lib.POL_DR_NPARAMS: wc._call("tsidb_policy_randomize", p.ctypes.data_as(vp) if p is not None else None, k)
    good = np.zeros(_lib.POL_DR_NPARAMS)
    good[_lib.POL_DR_PUSH_INTERVAL], good[_lib.POL_DR_PUSH_DURATION], good[_lib.POL_DR_PUSH_FORCE_HI] = 5, 2, 1.0

    def changed(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[getattr(_lib, "POL_DR_" + k)] = v
        return p
    bad = [changed(RESET_YAW=float("nan")), changed(NOISE_GRAVITY=float("inf")), changed(RESET_JOINT_POS=-0.1), changed(RESET_LIFT=-0.01),
           changed(PUSH_DURATION=6), changed(PUSH_FORCE_LO=2.0), changed(COMMAND_INTERVAL=-1), changed(COMMAND_ZERO_PROB=1.01),
           changed(COMMAND_ZERO_PROB=-0.01), changed(SEED=2.0 ** 32), changed(ENV_OFFSET=0.5), changed(PUSH_INTERVAL=2.0 ** 31)]
    for p in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_randomize"):
            randomize(p)
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_DR_NPARAMS"):
        randomize(good, _lib.POL_DR_NPARAMS - 1)
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_DR_NPARAMS"):
        randomize(None, 3)
    # nothing of the rejected vectors was taken: pushes are still off, a perturb launches nothing and needs no buffer
    assert wc.xfrc is None
    env._perturb()
    randomize(good)
    with pytest.raises(_lib.TsidbError, match="no xfrc buffer registered"):
        env._perturb()
    with pytest.raises(_lib.TsidbError, match="null buffer"):
        wc._call("tsidb_policy_reset_noise", C.byref(env._bufs), vp(wc.rows.data_ptr()), wc.NROW, None, vp(wc.qvel.data_ptr()), wc._stream())
    with pytest.raises(_lib.TsidbError, match="TSIDB_NROW"):
        wc._call("tsidb_policy_reset_noise", C.byref(env._bufs), vp(wc.rows.data_ptr()), 3, vp(wc.qpos.data_ptr()), vp(wc.qvel.data_ptr()), wc._stream())
    xfrc = torch.zeros(n, wc.NB, 6, dtype=wc.dtype, device=wc.device)
    xfrc[:, 1:] = 0.25                                     # (a caller's wrenches on other bodies stay)
    xfrc[:, 0, 3:] = 0.5
    wc.set_xfrc(xfrc)
    env._perturb()
    torch.cuda.synchronize()
    assert (xfrc[:, 1:] == 0.25).all() and (xfrc[:, 0, 3:] == 0.5).all() and (xfrc[:, 0, 2] == 0).all()
    wc.set_xfrc(None)
    randomize(None, 0)                                     # everything off again: the unrandomised environment
    env._perturb()
    zeros = torch.zeros(n, env.NA, dtype=wc.dtype, device=wc.device)
    for _ in range(3):
        a, b = env.step(zeros), plain.step(zeros)
        assert torch.equal(a[0], b[0]) and torch.equal(env.wc.qpos, plain.wc.qpos) and torch.equal(env.command, plain.command)
