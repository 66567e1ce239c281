"""The policy environment (PolicyEnv; tsidb_policy_act / _reward / _obs): what it costs around the sim steps, and against the
same environment logic written with torch ops.  Policy-steps/s, float64, position mode about the standing pose with small
random actions (the robots stay on their feet: the same contact work throughout), episodes of 200 steps so that restarts are
part of the load, of
  (a) sim     the bare wc.sim_steps(decimation) loop - what the sim alone takes
  (b) torch   TorchEnv below: clip / delay ring / filter, reward terms, termination, reset_done, bookkeeping of the restarted
              envs and the observation row as element-wise torch ops on the same tensors (commands are redrawn with torch.rand
              instead of the library's hash; everything else computes what the kernels compute)
  (c) fused   PolicyEnv.step
at 4096 and 512 envs, decimation 4 and 10, timed windows alternating between the three.
    python tools/policy_env.py [out.json]          (on an MI355X; default profiles/policy_env.json)
    python tools/policy_env.py --trace ENVS STEPS  (a short run of (c) alone, for rocprofv3 --kernel-trace --stats)
    python tools/policy_env.py --randomize [out.json]   (c) with every group of the randomisation on (PolicyRandomization: reset
              noise, observation noise, pushes of at most 1 N, command resampling) against (c) with it off, in alternating
              windows, at 4096 and 512 envs, decimation 4 and 10; default profiles/policy_dr.json
    python tools/policy_env.py --tsid stand|walk [--mode residual|motor|position] [out.json]   TSID in the loop (PolicyEnv(tsid=...),
              default mode residual) against the hand-driven closed loop over the same number of sim steps (wc.step, in "walk" behind
              sched.apply on a device clock), against the same env with the two teacher launches left out, and against the bare
              tsid=None env, in alternating windows, at 4096 and 512 envs, decimation 4; default profiles/policy_tsid.json (the file
              keeps one entry per (tsid, mode): a run replaces its own and leaves the others)
    python tools/policy_env.py --terrain [out.json]   per-episode terrain and dynamics and the height scan (PolicyEnv(terrain=...): a
              4 % mass range, friction 0.4 - 1, 5 degrees of tilt, steps of 0 - 1 cm, an 11 x 7 scan) against the env without them on
              tables drawn once on the host (wc.randomize(): the same sim path, no per-episode redraw, no scan), in alternating
              windows, at 4096 and 512 envs, decimation 4 and 10; default profiles/policy_terrain.json.  The two kernels' times come
              from a run of their own: rocprofv3 --kernel-trace --stats -- python tools/policy_env.py --terrain --trace ENVS STEPS
    python tools/policy_env.py --actor [out.json]   the policy in the loop: PolicyEnv.rollout with a PolicyActor (one fused launch per
              step: networks, sample, log-probability, value, written into the rollout storage) against TorchActor below - the same
              networks as nn.Sequential in float32 with cat, cast, torch.randn, log-prob, value, cast back and copies into the same
              storage - each eager and captured in a graph, in alternating windows of 16-step rollouts (a process per case), at 4096 and 512 envs,
              decimation 4; actor obs -> 256 -> 128 -> NA (ELU), critic obs | priv -> 256 -> 128 -> 1, and the same with obs |
              height_scan (77) as the actor's input; default profiles/policy_actor.json.  The kernel's time comes from a run of its
              own: rocprofv3 --kernel-trace --stats -- python tools/policy_env.py --actor --trace ENVS STEPS
    python tools/policy_env.py --learn [out.json]   one PPO update on a recorded 16-step rollout (5 epochs x 4 minibatches, Adam): PolicyLearner
              (three launches per minibatch: loss, backward and weight gradients on the storage's own rows) against TorchLearner below -
              the same loss in eager torch over nn.Sequential copies of the networks, the same minibatches, the same optimiser - in
              alternating windows (a process per case), at 4096 and 512 envs, the 256-128 networks; and the first minibatch's loss from
              both on equal weights; default profiles/policy_learner.json.  The kernels' times come from a run of its own:
              rocprofv3 --kernel-trace --stats -- python tools/policy_env.py --learn --trace ENVS UPDATES
    python tools/policy_env.py --actor --normalize [out.json]   --actor's "obs" case with a PolicyNormalizer in the fused actors (two
              more launches per step, the map inside the actor's) against TorchActor with a torch transcription of rsl_rl's
              EmpiricalNormalization in front of each network; --learn --normalize: --learn on a rollout recorded with the
              normaliser (the learner reads the stored, normalised rows; it does not change).  A process per case, four alternating
              windows, medians, 4096 and 512 envs; default profiles/policy_norm.json (one entry per mode: a run replaces its own).
              Kernel times: rocprofv3 --kernel-trace --stats -- python tools/policy_env.py --actor --normalize --trace ENVS STEPS
              (a rollout with the normaliser off, then one with it on)
    python tools/policy_env.py --learn --optimizer [out.json]   what follows the gradients in rsl_rl's PPO iteration - the adaptive
              step size from the exact KL, clip_grad_norm_, Adam - on --learn's recorded rollout, 5 epochs x 4 minibatches, updates/s of
              PolicyLearner with (plain) torch.optim.Adam alone, --learn's fused path; (a) clip_grad_norm_ + torch.optim.Adam + rsl_rl's
              rule with its host read of the KL; (b) the same with the rule written sync-free on a tensor lr (Adam capturable);
              (c) PolicyOptimizer; (d) (c) with the whole update() captured in one graph - each on a learner of its own over equal
              weights, in alternating windows (a process per case), at 4096 and 512 envs; default profiles/policy_optimizer.json.
              Kernel times: rocprofv3 --kernel-trace --stats -- python tools/policy_env.py --learn --optimizer --trace ENVS UPDATES
    python tools/policy_env.py --distill [--beta B --beta-decay D --iters K] [out.json]   imitation of the TSID teacher: a standing env
              with TSID beside the policy (tsid="stand", motor mode: an action is a torque), the 256-128 networks, K DAgger
              iterations at 512 envs - a 16-step teacher rollout at beta (RolloutStorage(teacher=True), rollout(teacher_beta=...)),
              2 epochs x 4 minibatches of pure distillation (PolicyLearner(imitation_coef=1, surrogate_coef=0, value_coef=0) with a
              PolicyOptimizer), beta *= D on the device - with L_im, the running episode length, the executed share and the restarts
              per iteration; `control`: the same rollouts with the untrained student alone; and, at 4096 x 16 and 512 x 16 rows,
              backward() with the term off (the parent commit's call) and on, and the 16-step rollout into a plain storage (the
              parent's launches), into a teacher storage, and with beta = 0.5, in alternating windows (a process per case);
              default profiles/policy_imitation.json.  Kernel times: rocprofv3 --kernel-trace --stats -- python
              tools/policy_env.py --distill --trace ENVS CALLS (CALLS backward() with the term off, then on)
    python tools/policy_env.py --episodes [out.json]   episode statistics and the terrain curriculum (PolicyEnv(curriculum=...): two
              launches per step) against the env without them and against the same bookkeeping with torch ops behind every step
              (TorchEpisodes below, which cannot see a fallen env's final position), in alternating windows, at 4096 and 512 envs,
              decimation 4; then the curriculum under TSID's own walk (tsid="walk", zero residual, eight levels of steps up to 4 cm, strips of 3 - 6 cm):
              the level histogram per iteration and the share of each level's episodes that went up; default
              profiles/policy_episode.json.  --episodes --curriculum: that second part alone.  Kernel times: rocprofv3 --kernel-trace
              --stats -- python tools/policy_env.py --episodes --trace ENVS STEPS
    python tools/policy_env.py --history H [out.json]   the observation history (PolicyEnv(obs_history=dict(frames=H, sources=("obs",))):
              one launch per step) against the env without it and against the same stack with torch ops behind every step
              (TorchHistory below: cat, where on done, repeat), in alternating windows, at 4096 and 512 envs, decimation 4; whether
              the two stacks end bit-identical; then eager 16-step rollouts of an actor on the stacked row against the same actor
              on obs alone (H x 71 <= 512); default profiles/policy_obs_history.json.  Kernel time: rocprofv3 --kernel-trace
              --stats -- python tools/policy_env.py --history H --trace ENVS STEPS (which prints the bytes a launch moves)
    python tools/policy_env.py --symmetry [out.json]   the learner's mirror symmetry (PolicyLearner(symmetry=PolicySymmetry(env, actor))):
              backward() on one minibatch of --learn's recorded rollout with augmentation alone, with the mirror term alone and with
              both, against the plain backward() and against the same loss in eager torch (gather, mirror, concatenate, autograd),
              in alternating windows, at 4096 x 16 and 512 x 16 rows (a process per case); the first minibatch's loss, L_sym and
              gradients from both; default profiles/policy_symmetry.json"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tsid_control_amd import PolicyEnv, RobotConfig, WalkController, _lib  # noqa: E402

WEIGHTS = dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-1.0, base_height=-10.0,
               action_rate=-0.01, joint_vel=-1e-3, feet_air_time=1.0, alive=0.2, termination=-5.0)
KW = dict(action_scale=0.25, action_clip=1.0, filter_alpha=0.8, command_range=((0.0, 0.5), (0.0, 0.0), (-0.5, 0.5)), max_episode_steps=200,
          reward_weights=WEIGHTS)


class TorchEnv:
    """PolicyEnv's step with torch ops in place of the three kernels"""

    def __init__(self, n, decimation, delay):
        conf = RobotConfig()
        conf.reference_quirks = False
        self.wc = wc = WalkController(conf, num_envs=n, device="cuda:0")
        z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
        wc.set_ctrl(z(n, wc.NA), "position")
        self.n, self.NA, self.decimation, self.delay = n, wc.NA, decimation, delay.long()
        self.hist, self.last, self.prev = z(8, n, wc.NA), z(n, wc.NA), z(n, wc.NA)
        self.command, self.air = z(n, 3), z(n, 2)
        self.ep_len, self.episode = z(n, dt=torch.int64), z(n, dt=torch.int64)
        self.default = wc.ctrl_from_q(wc.q0)[0].clone()
        self.scale, self.clip, self.alpha, self.sigma2 = 0.25, 1.0, 0.8, 0.25 ** 2
        self.h_target, self.t_air, self.deadband, self.max_steps = float(wc.qpos[0, 2]), 0.25, 0.1, 200
        self.air_dt = decimation * conf.dt
        self.w = torch.tensor([WEIGHTS.get(k, 0.0) for k in _lib.POL_TERMS], dtype=wc.dtype, device=wc.device)
        self.dof = torch.as_tensor(np.asarray(wc.model["mj_act_dof"], dtype=np.int64), device=wc.device)
        self.geom_body = torch.as_tensor(np.asarray(wc.model["mj_geom_body"], dtype=np.int64), device=wc.device)
        self.feet = (wc._named_site("lf_imu")[0], wc._named_site("rf_imu")[0])
        self.env_idx = torch.arange(n, device=wc.device)
        self.lo = torch.tensor([0.0, 0.0, -0.5], dtype=wc.dtype, device=wc.device)
        self.hi = torch.tensor([0.5, 0.0, 0.5], dtype=wc.dtype, device=wc.device)
        self.done_height, self.done_tilt = 0.2, float(np.cos(np.deg2rad(45.0)))
        self.obs = z(n, 11 + 3 * wc.NA + 4)

    def rot(self):
        q = self.wc.qpos[:, 3:7]
        q = q / q.norm(dim=1, keepdim=True)
        w, x, y, z = q.unbind(1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                            2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)

    def contacts(self):
        wc = self.wc
        cp = wc.con_pairs.long()
        live = (torch.arange(32, device=cp.device)[None, :] < wc.ncon[:, None]) & (cp >= 0) & ((cp & 0x8000) == 0)
        body = self.geom_body[torch.where(live, cp >> 16, torch.zeros_like(cp))]
        foot = torch.stack([(live & (body == b)).any(1) for b in self.feet], dim=1)
        return foot, (live & (body == 0)).any(1)

    def step(self, action):
        wc = self.wc
        # act
        act = action.clamp(-self.clip, self.clip)
        self.hist[self.ep_len & 7, self.env_idx] = act
        delayed = self.hist[(self.ep_len - self.delay) & 7, self.env_idx]
        delayed = torch.where((self.delay > self.ep_len)[:, None], torch.zeros_like(delayed), delayed)
        target = self.default + self.scale * delayed
        wc.ctrl += self.alpha * (target - wc.ctrl)
        self.prev.copy_(self.last)
        self.last.copy_(act)
        wc.sim_steps(self.decimation)
        # reward
        R = self.rot()
        v = torch.einsum("nji,nj->ni", R, wc.qvel[:, 0:3])
        om, cmd = wc.qvel[:, 3:6], self.command
        foot, torso = self.contacts()
        first = foot & (self.air > 0)
        moving = cmd[:, :2].norm(dim=1) > self.deadband
        finite = torch.isfinite(wc.qpos).all(1) & torch.isfinite(wc.qvel).all(1)
        up = 1 - 2 * (wc.qpos[:, 4] ** 2 + wc.qpos[:, 5] ** 2)
        term = ((wc.info[:, 3] & 4) != 0) | ~finite | (wc.qpos[:, 2] < self.done_height) | (up < self.done_tilt) | torso
        timeout = ~term & (self.ep_len + 1 >= self.max_steps)
        terms = torch.stack([torch.exp(-((cmd[:, :2] - v[:, :2]) ** 2).sum(1) / self.sigma2), torch.exp(-(cmd[:, 2] - om[:, 2]) ** 2 / self.sigma2),
                             v[:, 2] ** 2, (om[:, :2] ** 2).sum(1), (R[:, 2, :2] ** 2).sum(1), (wc.qpos[:, 2] - self.h_target) ** 2,
                             torch.zeros_like(up), ((self.last - self.prev) ** 2).sum(1), (wc.qvel[:, self.dof] ** 2).sum(1),
                             (torch.where(first, self.air - self.t_air, torch.zeros_like(self.air)).sum(1) * moving),
                             torch.ones_like(up), term.to(up.dtype)], dim=1)
        self.air = torch.where(foot, torch.zeros_like(self.air), self.air + self.air_dt)
        wc.reward.copy_(terms @ self.w)
        done = term | timeout
        wc.done.copy_(done.to(wc.dtype))
        self.ep_len += 1
        wc.reset_done()
        # restarted envs, observation
        keep = (~done)[:, None].to(wc.dtype)
        self.hist *= keep[None]
        self.last *= keep
        self.prev *= keep
        self.air *= keep
        self.ep_len *= ~done
        self.episode += done
        wc.ctrl.copy_(torch.where(done[:, None], self.default[None, :], wc.ctrl))
        self.command = torch.where(done[:, None], self.lo + (self.hi - self.lo) * torch.rand_like(self.command), self.command)
        R = self.rot()
        foot = self.contacts()[0] | done[:, None]
        self.obs = torch.cat([wc.qvel[:, 3:6], -R[:, 2, :], self.command, wc.qpos[:, self.dof + 1] - self.default, wc.qvel[:, self.dof],
                              self.last, foot.to(wc.dtype), torch.einsum("nji,nj->ni", R, wc.qvel[:, 0:3]), wc.qpos[:, 2:3]], dim=1)
        return self.obs, wc.reward, wc.done


def alternate(run, window, windows, preroll, per_call=1):
    """run: {name: fn(k), k calls}.  `preroll` calls of each, then `windows` rounds of one timed window of `window` calls per runner,
    the order rotating by one per round.  Returns the first keys of every result: policy-steps/s (`per_call` steps a call) as
    medians and window by window, and the medians as microseconds per policy step"""
    for fn in run.values():
        fn(preroll)
    torch.cuda.synchronize()
    res = {k: [] for k in run}
    order = list(run)
    for w in range(windows):
        first = w % len(order)
        for name in order[first:] + order[:first]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[name](window)
            torch.cuda.synchronize()
            res[name].append(window * per_call / (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in res.items()}
    return dict(policy_steps_per_s_median=med, all=res, us_per_policy_step={k: 1e6 / v for k, v in med.items()})


def delays(n):
    return (torch.arange(n, dtype=torch.int32, device="cuda:0") % 3).contiguous()


def stepper(env, n, na):
    """fn(k): k steps of env under 16 small random actions in turn (the same 16 for every env)"""
    g = torch.Generator(device="cuda:0").manual_seed(1)
    actions = [(torch.rand(n, na, generator=g, dtype=torch.float64, device="cuda:0") - 0.5) * 0.2 for _ in range(16)]
    return lambda k: [env.step(actions[i & 15]) for i in range(k)]


def report(out_path, **out):
    """the result as JSON, printed and written to out_path"""
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), dtype="f64", **out), indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


def measure(n, decimation, window=300, windows=4, preroll=60):
    delay = delays(n)
    fused = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **KW)
    eager = TorchEnv(n, decimation, delay)
    bare_conf = RobotConfig()
    bare_conf.reference_quirks = False
    bare = WalkController(bare_conf, num_envs=n, device="cuda:0")
    bare.set_ctrl(bare.ctrl_from_q(bare.q0).expand(n, -1).contiguous(), "position")
    r = alternate(dict(sim=lambda k: [bare.sim_steps(decimation) for _ in range(k)], torch=stepper(eager, n, fused.NA),
                       fused=stepper(fused, n, fused.NA)), window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    return dict(envs=n, decimation=decimation, window_policy_steps=window, windows=windows, **r, fused_overhead_over_sim_us=us["fused"] - us["sim"], torch_overhead_over_sim_us=us["torch"] - us["sim"],
                fused_vs_torch=med["fused"] / med["torch"], restarts_fused=int(fused.episode.sum()) - n, restarts_torch=int(eager.episode.sum()),
                standing_height_min=float(fused.wc.qpos[:, 2].min()))


RANDOMIZATION = dict(seed=1, reset_joint_pos=0.05, reset_joint_vel=0.2, reset_base_lin_vel=0.1, reset_base_ang_vel=0.2, reset_yaw=np.pi,
                     reset_xy=0.5, reset_lift=0.005, noise_ang_vel=0.2, noise_gravity=0.05, noise_joint_pos=0.01, noise_joint_vel=1.5,
                     push_interval=50, push_duration=5, push_force_lo=0.2, push_force_hi=1.0, command_interval=100, command_zero_prob=0.1)


def measure_randomize(n, decimation, window=300, windows=4, preroll=60):
    """(c) with everything on against (c) with everything off: policy-steps/s in alternating windows of one process"""
    delay = delays(n)
    envs = dict(off=PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **KW),
                on=PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, randomization=RANDOMIZATION, **KW))
    r = alternate({k: stepper(e, n, e.NA) for k, e in envs.items()}, window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    return dict(envs=n, decimation=decimation, window_policy_steps=window, windows=windows, **r, on_over_off=med["on"] / med["off"], randomisation_us_per_policy_step=us["on"] - us["off"],
                restarts={k: int(e.episode.sum()) - n for k, e in envs.items()},
                standing_height_min={k: float(e.wc.qpos[:, 2].min()) for k, e in envs.items()})


TERRAIN = dict(seed=1, mass=(0.98, 1.02), friction=(0.4, 1.0), tilt_deg=5.0, step_height=(0.0, 0.01), step_length=(0.04, 0.12), step_prob=0.5,
               flat_cells=1, num_levels=1, scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7), scan_clip=(-0.2, 0.6), scan_noise=0.01)


def measure_terrain(n, decimation, window=300, windows=4, preroll=60):
    """host: tables drawn once with wc.randomize() (what the library offered before); device: PolicyEnv(terrain=TERRAIN).
    Policy-steps/s in alternating windows of one process"""
    delay = delays(n)
    envs = dict(host=PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **KW),
                device=PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, terrain=TERRAIN, **KW))
    envs["host"].wc.randomize(seed=1, mass=TERRAIN["mass"], friction=TERRAIN["friction"], tilt_deg=TERRAIN["tilt_deg"],
                              step_height=TERRAIN["step_height"][1], step_length=TERRAIN["step_length"])
    r = alternate({k: stepper(e, n, e.NA) for k, e in envs.items()}, window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    return dict(envs=n, decimation=decimation, window_policy_steps=window, windows=windows, **r, device_over_host=med["device"] / med["host"], terrain_us_per_policy_step=us["device"] - us["host"],
                restarts={k: int(e.episode.sum()) - n for k, e in envs.items()},
                height_min={k: float(e.wc.qpos[:, 2].min()) for k, e in envs.items()},
                scan_min_max=[float(envs["device"].height_scan.min()), float(envs["device"].height_scan.max())])


TEACH = dict(track_com=1.0, track_feet=1.0, contact_match=0.25, deviation=-0.01)


class NoTeacher(PolicyEnv):
    """the tsid env without its two teacher launches: what they add is the difference to the full env"""

    def _teacher(self):
        pass

    def _teacher_obs(self):
        pass


def measure_tsid(n, tsid, mode, decimation=4, window=100, windows=4, preroll=20):
    """policy-steps/s of hand (the closed loop alone), tsid (PolicyEnv with TSID in the loop), noteacher (that without the two
    new launches) and bare (tsid=None, position mode: tsidb_sim_ctrl only), in alternating windows of one process"""
    from tsid_control_amd.walk_planner import WalkSchedule, op3_closed_loop_walking_conf, op3_walking_posture
    delay = delays(n)

    def conf():
        c = op3_closed_loop_walking_conf(RobotConfig()) if tsid == "walk" else RobotConfig()
        c.closed_loop, c.reference_quirks = True, False
        return c

    kw = dict(KW, action_scale=dict(residual=0.05, motor=0.3, position=0.25)[mode])
    make = lambda cls: cls(conf(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, tsid=tsid, mode=mode, teacher_weights=TEACH, **kw)
    envs = dict(tsid=make(PolicyEnv), noteacher=make(NoTeacher),
                bare=PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **KW))
    hand = WalkController(conf(), num_envs=n, device="cuda:0")
    dt = hand.conf.dt
    if tsid == "walk":
        hand.set_posture_bias(op3_walking_posture())
        clock = torch.zeros(1, dtype=torch.float64, device=hand.device)
        sched = WalkSchedule.on_device(hand, foot_press=0.0)
        sched.enable_touchdown_feedback()

        def hand_step():
            for _ in range(decimation):
                sched.apply(hand, 0.0, t_device=clock)
                hand.step(1)
                clock.add_(dt)
    else:
        hand_step = lambda: hand.step(decimation)
    r = alternate(dict(hand=lambda k: [hand_step() for _ in range(k)], **{k: stepper(e, n, hand.NA) for k, e in envs.items()}),
                  window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    return dict(envs=n, tsid=tsid, mode=mode, decimation=decimation, window_policy_steps=window, windows=windows, **r, tsid_over_hand=med["tsid"] / med["hand"], tsid_over_bare=med["tsid"] / med["bare"],
                policy_layer_us_per_policy_step=us["tsid"] - us["hand"], teacher_launches_us_per_policy_step=us["tsid"] - us["noteacher"],
                restarts={k: int(e.episode.sum()) - n for k, e in envs.items()}, failed_qp_hand=int((hand.status != 0).sum()),
                height_min={k: float(e.wc.qpos[:, 2].min()) for k, e in envs.items()})


def actor_nets(env, scan, seed=1):
    """(actor, critic, actor_inputs, critic_inputs, log_std) of the --actor measurement, float32 on the env's device"""
    torch.manual_seed(seed)
    k = env.NOBS + (77 if scan else 0)
    mlp = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, 256), torch.nn.ELU(), torch.nn.Linear(256, 128), torch.nn.ELU(),
                                           torch.nn.Linear(128, o)).to(env.device)
    return (mlp(k, env.NA), mlp(env.NOBS + 4, 1), ("obs", "height_scan") if scan else ("obs",), ("obs", "priv"),
            torch.full((env.NA,), -2.0, dtype=torch.float32, device=env.device))


class TorchNormalizer:
    """rsl_rl's EmpiricalNormalization, transcribed: float32 buffers, update() then (x - mean) / (std + eps)"""

    def __init__(self, k, device, eps=1e-2):
        self.eps = eps
        self.mean, self.var, self.std = torch.zeros(1, k, device=device), torch.ones(1, k, device=device), torch.ones(1, k, device=device)
        self.count = torch.zeros((), device=device)     # (a device tensor and in-place updates: a captured graph keeps counting)

    def __call__(self, x, update=True):
        if update:
            n = x.shape[0]
            self.count.add_(n)
            rate = n / self.count
            var_x, mean_x = torch.var(x, dim=0, unbiased=False, keepdim=True), torch.mean(x, dim=0, keepdim=True)
            delta = mean_x - self.mean
            mean = self.mean + rate * delta
            self.var.add_(rate * (var_x - self.var + delta * (mean_x - mean)))
            self.mean.copy_(mean)
            self.std.copy_(torch.sqrt(self.var))
        return (x - self.mean) / (self.std + self.eps)


class TorchActor:
    """PolicyActor and PolicyEnv.rollout with torch ops in place of the fused launch, into the same RolloutStorage; normalize:
    a TorchNormalizer in front of each network, updated per step and not by the closing value (PolicyNormalizer's order)"""

    def __init__(self, env, actor, critic, actor_inputs, critic_inputs, log_std, normalize=False):
        self.env, self.actor, self.critic, self.log_std = env, actor, critic, log_std
        self.ai, self.ci = [getattr(env, k) for k in actor_inputs], [getattr(env, k) for k in critic_inputs]
        width = lambda blocks: sum(b.shape[1] for b in blocks)
        self.norm = (TorchNormalizer(width(self.ai), env.device), TorchNormalizer(width(self.ci), env.device)) if normalize else None

    @torch.no_grad()
    def rollout(self, steps, st):
        env, ls = self.env, self.log_std
        for t in range(steps):
            x, xc = torch.cat(self.ai, dim=1).float(), torch.cat(self.ci, dim=1).float()
            if self.norm:
                x, xc = self.norm[0](x), self.norm[1](xc)
            mean = self.actor(x)
            eps = torch.randn_like(mean)
            a = mean + ls.exp() * eps
            st.logp[t].copy_(-(0.5 * eps * eps + ls).sum(1) - 0.5 * env.NA * 1.8378770664093453)
            st.value[t].copy_(self.critic(xc).squeeze(1))
            st.actor_input[t].copy_(x); st.critic_input[t].copy_(xc); st.action[t].copy_(a); st.mean[t].copy_(mean)
            env.step(a.to(env.dtype))
            st.reward[t].copy_(env.reward); st.done[t].copy_(env.done); st.timeout[t].copy_(env.timeout)
        xc = torch.cat(self.ci, dim=1).float()
        st.value[steps].copy_(self.critic(self.norm[1](xc, update=False) if self.norm else xc).squeeze(1))
        return st


def captured(fn):
    """fn captured in a graph after a warm-up on a side stream; returns the replay.  The replay keeps fn alive, and with it every
    tensor the captured launches read and write (the actor's parameters and outputs, the storage: rollout_written()) - a graph
    holds addresses, not references"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return lambda keep=fn: g.replay()


def measure_actor(n, scan, decimation=4, steps=16, window=10, windows=4, preroll=3, normalize=False):
    """policy-steps/s of 16-step rollouts: fused / torch, each eager and graph-captured, in alternating windows of one process;
    normalize: a PolicyNormalizer in the fused actors, TorchNormalizers in the torch ones"""
    from tsid_control_amd import PolicyActor, PolicyNormalizer, RolloutStorage
    delay = delays(n)
    kw = dict(KW, action_scale=0.05, terrain=TERRAIN) if scan else dict(KW, action_scale=0.05)
    run, envs = {}, {}
    for name in ("fused", "fused_graph", "torch", "torch_graph"):
        env = envs[name] = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **kw)
        actor, critic, ai, ci, ls = actor_nets(env, scan)
        fused_norm = PolicyNormalizer() if normalize and name.startswith("fused") else None
        pa = PolicyActor(env, actor, critic, actor_inputs=ai, critic_inputs=ci, log_std=ls, normalizer=fused_norm)
        st = RolloutStorage(env, pa, steps)
        if name.startswith("fused"):
            fn = lambda env=env, pa=pa, st=st: env.rollout(pa, steps, st)
        else:
            ta = TorchActor(env, actor, critic, ai, ci, ls, normalize=normalize)
            fn = lambda ta=ta, st=st: ta.rollout(steps, st)
        fn = captured(fn) if name.endswith("graph") else fn
        run[name] = lambda k, fn=fn: [fn() for _ in range(k)]
    r = alternate(run, window, windows, preroll, per_call=steps)
    med = r["policy_steps_per_s_median"]
    return dict(envs=n, actor_input="obs | height_scan" if scan else "obs", normalize=normalize, decimation=decimation, rollout_steps=steps,
                window_rollouts=window, windows=windows, **r, fused_over_torch=med["fused"] / med["torch"], fused_graph_over_torch_graph=med["fused_graph"] / med["torch_graph"],
                fused_over_torch_graph=med["fused"] / med["torch_graph"],
                restarts={k: int(e.episode.sum()) - n for k, e in envs.items()},
                height_min={k: float(e.wc.qpos[:, 2].min()) for k, e in envs.items()})


class TorchLearner:
    """PolicyLearner's loss and update in eager torch with autograd: nn.Sequential copies of the two networks and of log_std, the
    forward pass over the storage's own rows"""

    def __init__(self, actor, critic, log_std, clip=0.2, value_coef=1.0, entropy_coef=0.0):
        import copy
        self.actor, self.critic = copy.deepcopy(actor), copy.deepcopy(critic)
        self.log_std = log_std.clone().requires_grad_()
        self.clip, self.value_coef, self.entropy_coef = clip, value_coef, entropy_coef
        self.adv_stats = None

    def parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + [self.log_std]

    def loss(self, st, index):
        rows, c, ls = st.logp.numel(), self.clip, self.log_std
        j = index.long()
        flat = lambda t: t.reshape(rows, -1)[j]
        mu, v = self.actor(flat(st.actor_input)), self.critic(flat(st.critic_input)).squeeze(1)
        z = (flat(st.action) - mu) / ls.exp()
        logp = -(0.5 * z * z + ls).sum(1) - 0.5 * mu.shape[1] * 1.8378770664093453
        r = (logp - st.logp.reshape(-1)[j]).exp()
        adv = (st.advantage.reshape(-1)[j] - self.adv_stats[0]) * self.adv_stats[1]
        l_pi = torch.max(-adv * r, -adv * r.clamp(1 - c, 1 + c)).mean()
        old, ret = st.value[:-1].reshape(-1)[j], st.returns.reshape(-1)[j]
        l_v = torch.max((v - ret) ** 2, (old + (v - old).clamp(-c, c) - ret) ** 2).mean()
        entropy = (ls + 0.5 * (1 + 1.8378770664093453)).sum()
        return l_pi + self.value_coef * l_v - self.entropy_coef * entropy

    def update(self, st, opt, epochs, minibatches, generator):
        rows = st.logp.numel()
        self.adv_stats = torch.stack([st.advantage.mean(), 1.0 / (st.advantage.std() + 1e-8)])
        for _ in range(epochs):
            perm = torch.randperm(rows, generator=generator, dtype=torch.int32, device=st.logp.device)
            for k in range(minibatches):
                opt.zero_grad(set_to_none=True)
                self.loss(st, perm[k * rows // minibatches:(k + 1) * rows // minibatches]).backward()
                opt.step()


def learn_setup(n, steps=16, decimation=4, normalize=False):
    """(storage with its advantages, PolicyLearner, TorchLearner on copies of the same weights) after one recorded rollout;
    normalize: recorded with a PolicyNormalizer, so both learners read the normalised rows the storage holds"""
    from tsid_control_amd import PolicyActor, PolicyLearner, PolicyNormalizer
    env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delays(n), **dict(KW, action_scale=0.05))
    actor, critic, ai, ci, ls = actor_nets(env, False)
    pa = PolicyActor(env, actor, critic, actor_inputs=ai, critic_inputs=ci, log_std=ls, normalizer=PolicyNormalizer() if normalize else None)
    st = env.rollout(pa, steps)
    st.gae(0.99, 0.95)
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01)
    return st, PolicyLearner(pa, **kw), TorchLearner(actor, critic, ls, **kw)


def measure_learn(n, epochs=5, minibatches=4, window=40, windows=4, preroll=3, normalize=False):
    """updates/s of one PPO update on the same recorded rollout: fused / torch in alternating windows of one process, and the
    loss of the first minibatch from both before either has moved a weight"""
    st, fused, eager = learn_setup(n, normalize=normalize)
    rows = st.logp.numel()
    index = torch.randperm(rows, generator=torch.Generator(device="cuda:0").manual_seed(3), dtype=torch.int32, device="cuda:0")[:rows // minibatches]
    stats = fused.backward(st, index).clone()
    eager.adv_stats = fused.adv_stats.clone()
    with torch.no_grad():
        loss_torch = float(eager.loss(st, index))
    grad_torch = torch.autograd.grad(eager.loss(st, index), eager.parameters())
    grad_rel = max(float((a.grad - b).abs().max() / b.abs().max()) for a, b in zip(fused.parameters(), grad_torch))
    opts = dict(fused=torch.optim.Adam(fused.parameters(), lr=1e-4), torch=torch.optim.Adam(eager.parameters(), lr=1e-4))
    gens = {k: torch.Generator(device="cuda:0").manual_seed(5) for k in opts}
    run = dict(fused=lambda k: [fused.update(st, opts["fused"], epochs, minibatches, gens["fused"]) for _ in range(k)],
               torch=lambda k: [eager.update(st, opts["torch"], epochs, minibatches, gens["torch"]) for _ in range(k)])
    r = alternate(run, window, windows, preroll)
    med = r["policy_steps_per_s_median"]
    last = fused.update(st, opts["fused"], 1, minibatches, gens["fused"])
    return dict(envs=n, normalize=normalize, rollout_steps=st.steps, rows=rows, epochs=epochs, minibatches=minibatches, minibatch_rows=rows // minibatches,
                window_updates=window, windows=windows, updates_per_s_median=med, updates_per_s_all=r["all"],
                ms_per_update={k: 1e3 / v for k, v in med.items()}, fused_over_torch=med["fused"] / med["torch"],
                first_minibatch=dict(loss_fused=float(stats[5]), loss_torch=loss_torch, loss_difference=float(stats[5]) - loss_torch,
                                     largest_gradient_difference_over_largest_entry=grad_rel,
                                     stats=dict(zip(_lib.POL_LEARN_STATS, (float(x) for x in stats)))),
                stats_after=dict(zip(_lib.POL_LEARN_STATS, (float(x) for x in last[-1]))))


OPT = dict(lr=1e-3, desired_kl=0.01, max_grad_norm=1.0, lr_min=1e-5, lr_max=1e-2)      # rsl_rl's defaults


def torch_kl(st, learner, index, log_std_old):
    """rsl_rl's KL between the rollout's policy and the current one on the minibatch of the learner's last backward(), torch ops"""
    mu = learner.outputs(int(index.shape[0]))[0]
    old = st.mean.reshape(-1, mu.shape[1])[index.long()]
    s = learner.actor.log_std
    return (s - log_std_old + (torch.exp(2 * log_std_old) + (old - mu) ** 2) / (2 * torch.exp(2 * s)) - 0.5).sum(1).mean()


def torch_update(st, learner, adam, epochs, minibatches, generator, host_read):
    """PolicyLearner.update()'s loop with what rsl_rl runs between the gradients and the step in torch: the adaptive rule - with
    its host read of the KL, or sync-free on the tensor adam holds as lr - clip_grad_norm_, adam.step()"""
    rows, d = st.logp.numel(), OPT["desired_kl"]
    learner.fill_adv_stats(st)
    log_std_old = learner.actor.log_std.detach().clone()
    params, group = learner.parameters(), adam.param_groups[0]
    for _ in range(epochs):
        perm = torch.randperm(rows, generator=generator, dtype=torch.int32, device=st.logp.device)
        for k in range(minibatches):
            index = perm[k * rows // minibatches:(k + 1) * rows // minibatches]
            learner.backward(st, index, adv_stats=learner.adv_stats)
            kl = torch_kl(st, learner, index, log_std_old)
            lr = group["lr"]
            if host_read:
                kl = float(kl)
                if kl > 2 * d:
                    group["lr"] = max(OPT["lr_min"], lr / 1.5)
                elif 0 < kl < d / 2:
                    group["lr"] = min(OPT["lr_max"], lr * 1.5)
            else:
                lr.copy_(torch.where(kl > 2 * d, (lr / 1.5).clamp(min=OPT["lr_min"]),
                                     torch.where((kl > 0) & (kl < d / 2), (lr * 1.5).clamp(max=OPT["lr_max"]), lr)))
            torch.nn.utils.clip_grad_norm_(params, OPT["max_grad_norm"])
            adam.step()


def measure_optimizers(n, epochs=5, minibatches=4, window=40, windows=4, preroll=3):
    """updates/s of one PPO update on the same recorded rollout (a learner, a storage and weights of its own per runner, equal at
    the start): plain / a / b / c / d of this file's header, in alternating windows of one process"""
    from tsid_control_amd import PolicyOptimizer
    names = ("plain", "a_torch_host_read", "b_torch_tensor_lr", "c_policy_optimizer", "d_policy_optimizer_graph")
    sets = {k: learn_setup(n)[:2] for k in names}
    dev = "cuda:0"
    gens = {k: torch.Generator(device=dev).manual_seed(5) for k in names}
    adam = dict(plain=torch.optim.Adam(sets["plain"][1].parameters(), lr=1e-4),
                a_torch_host_read=torch.optim.Adam(sets["a_torch_host_read"][1].parameters(), lr=OPT["lr"]),
                b_torch_tensor_lr=torch.optim.Adam(sets["b_torch_tensor_lr"][1].parameters(), lr=torch.tensor(OPT["lr"], device=dev), capturable=True))
    fused = {k: PolicyOptimizer(sets[k][1], **OPT) for k in names[3:]}
    up = lambda k, opt, gen: sets[k][1].update(sets[k][0], opt, epochs, minibatches, gen)
    run = dict(plain=lambda c: [up("plain", adam["plain"], gens["plain"]) for _ in range(c)],
               a_torch_host_read=lambda c: [torch_update(*sets["a_torch_host_read"], adam["a_torch_host_read"], epochs, minibatches, gens["a_torch_host_read"], True)
                                            for _ in range(c)],
               b_torch_tensor_lr=lambda c: [torch_update(*sets["b_torch_tensor_lr"], adam["b_torch_tensor_lr"], epochs, minibatches, gens["b_torch_tensor_lr"], False)
                                            for _ in range(c)],
               c_policy_optimizer=lambda c: [up("c_policy_optimizer", fused["c_policy_optimizer"], gens["c_policy_optimizer"]) for _ in range(c)])
    capture = "held"
    try:                                   # the whole update() - randperm on the default generator included - as one graph
        k = names[4]
        up(k, fused[k], None)              # (the workspaces and every .grad exist before the capture)
        replay = captured(lambda: up(k, fused[k], None))
        run[k] = lambda c: [replay() for _ in range(c)]
    except Exception as e:                 # noqa: BLE001 - reported, the other four are measured without it
        capture = f"failed: {type(e).__name__}: {e}"
    r = alternate(run, window, windows, preroll)
    med = r["policy_steps_per_s_median"]
    c = fused["c_policy_optimizer"]
    c.log = torch.zeros(epochs * minibatches, 8, dtype=torch.float32, device=dev)
    up("c_policy_optimizer", c, gens["c_policy_optimizer"])
    log = c.log.cpu().numpy()
    return dict(envs=n, rows=sets["plain"][0].logp.numel(), epochs=epochs, minibatches=minibatches, minibatch_rows=sets["plain"][0].logp.numel() // minibatches,
                parameters=c.P, settings=OPT, window_updates=window, windows=windows, graph_capture=capture, updates_per_s_median=med,
                updates_per_s_all=r["all"], ms_per_update={k: 1e3 / v for k, v in med.items()},
                ms_per_update_over_plain={k: 1e3 / v - 1e3 / med["plain"] for k, v in med.items()},
                lr_after=dict(a_torch_host_read=float(adam["a_torch_host_read"].param_groups[0]["lr"]), b_torch_tensor_lr=float(adam["b_torch_tensor_lr"].param_groups[0]["lr"]),
                              c_policy_optimizer=float(c.lr)),
                last_update_of_c={name: [float(x) for x in log[:, i]] for i, name in enumerate(_lib.POL_OPT_STATS)})


def main_optimizer(args):
    """--learn --optimizer: a process per env count, results to profiles/policy_optimizer.json"""
    import subprocess
    if args and args[0] == "--trace":
        from tsid_control_amd import PolicyOptimizer
        st, fused, _ = learn_setup(int(args[1]))
        opt = PolicyOptimizer(fused, **OPT)
        for _ in range(int(args[2])):
            fused.update(st, opt, 5, 4)
        torch.cuda.synchronize()
        return
    if args and args[0] == "--case":
        print(json.dumps(measure_optimizers(int(args[1]))))
        return
    out_path = args[0] if args else "profiles/policy_optimizer.json"
    runs = []
    for n in (4096, 512):
        r = subprocess.run([sys.executable, sys.argv[0], "--learn", "--optimizer", "--case", str(n)], capture_output=True, text=True, check=True)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    report(out_path, actor="obs -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU",
           loss="clip 0.2, value_coef 1, entropy_coef 0.01, clipped value loss, normalised advantages", runs=runs)


def distill_env(n, decimation=4):
    """the standing env of --distill: TSID beside the policy in motor mode, an action = a torque [N m]"""
    conf = RobotConfig()
    conf.closed_loop, conf.reference_quirks = True, False
    return PolicyEnv(conf, num_envs=n, device="cuda:0", decimation=decimation, tsid="stand", mode="motor", action_scale=1.0, action_clip=100.0,
                     max_episode_steps=200, reward_weights=dict(alive=0.2, termination=-5.0), seed=1)


def distill_actor(env):
    from tsid_control_amd import PolicyActor
    actor, critic, ai, ci, ls = actor_nets(env, False)
    return PolicyActor(env, actor, critic, actor_inputs=ai, critic_inputs=ci, log_std=ls)


def run_distill(n, beta, decay, iters, steps=16, epochs=2, minibatches=4, learn=True):
    """DAgger with the TSID teacher: per iteration a `steps`-step teacher rollout at the current beta, `epochs` x `minibatches` pure
    distillation steps (PolicyOptimizer, constant lr 1e-3), beta *= decay on the device; per iteration L_im of the last
    minibatch, the mean length of the episodes that ended in the rollout (None: none ended), the share of rows the teacher's
    action was executed on, and the restarts.  learn = False: the control - the same rollouts with the untrained student alone
    (beta as given, no update), for the restarts a student that learns nothing has"""
    from tsid_control_amd import PolicyLearner, PolicyOptimizer, RolloutStorage
    env = distill_env(n)
    pa = distill_actor(env)
    st = RolloutStorage(env, pa, steps, teacher=True)
    pl = PolicyLearner(pa, imitation_coef=1.0, surrogate_coef=0.0, value_coef=0.0, entropy_coef=0.0)
    opt = PolicyOptimizer(pl, lr=1e-3)
    b = torch.full((1,), float(beta), dtype=torch.float32, device=env.device)
    rows = []
    for it in range(iters):
        before = env.episode.clone()
        env.rollout(pa, steps, st, teacher_beta=b)
        st.gae(0.99, 0.95)
        out = pl.update(st, opt, epochs, minibatches) if learn else torch.full((1, 8), float("nan"))
        if not learn:
            pl.backward(st, torch.arange(n * steps, dtype=torch.int32, device=env.device))       # (L_im of the whole rollout, no step)
        ended = st.done != 0
        rows.append(dict(iteration=it, beta=float(b), imitation_loss=float(pl.imit_stats[0]), loss=float(out[-1, 5]),
                         executed_share=float(st.teacher_executed.float().mean()), labelled_share=float(st.teacher_weight.mean()),
                         restarts=int((env.episode - before).sum()), ended_by_timeout=int(st.timeout.sum()), rows_done=int(ended.sum()),
                         mean_episode_length_running=float(env.ep_len.float().mean())))
        b.mul_(decay)
    return dict(envs=n, learn=learn, rollout_steps=steps, epochs=epochs, minibatches=minibatches, beta=beta, beta_decay=decay, iterations=rows)


def time_distill(n, steps=16, window=40, windows=4, preroll=3):
    """backward() at n x `steps` rows with the term off (tsidb_policy_learn: the parent commit's call) and on (pure distillation and
    PPO + term), and the 16-step rollout into a plain storage (the parent's launches), into a teacher storage without a beta (the
    same actions executed: the new launch is the only difference) and with beta = 0.5, in alternating windows of one process"""
    from tsid_control_amd import PolicyLearner, RolloutStorage
    env = distill_env(n)
    pa = distill_actor(env)
    st = env.rollout(pa, steps, RolloutStorage(env, pa, steps, teacher=True), teacher_beta=0.5)
    st.gae(0.99, 0.95)
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01)
    learners = dict(off=PolicyLearner(pa, **kw), ppo_bc=PolicyLearner(pa, imitation_coef=0.5, **kw),
                    distill=PolicyLearner(pa, imitation_coef=1.0, surrogate_coef=0.0, value_coef=0.0, entropy_coef=0.0))
    index = torch.randperm(n * steps, generator=torch.Generator(device="cuda:0").manual_seed(3), dtype=torch.int32, device="cuda:0")
    for pl in learners.values():
        pl.fill_adv_stats(st)
    back = alternate({k: (lambda c, pl=pl: [pl.backward(st, index, adv_stats=pl.adv_stats) for _ in range(c)]) for k, pl in learners.items()},
                     window, windows, preroll)
    plain = RolloutStorage(env, pa, steps)
    beta = torch.full((1,), 0.5, dtype=torch.float32, device=env.device)
    roll = alternate(dict(plain=lambda c: [env.rollout(pa, steps, plain) for _ in range(c)],
                          labels=lambda c: [env.rollout(pa, steps, st) for _ in range(c)],
                          mixed=lambda c: [env.rollout(pa, steps, st, teacher_beta=beta) for _ in range(c)]), max(2, window // 4), windows, 1)
    us = lambda r: {k: 1e6 / v for k, v in r["policy_steps_per_s_median"].items()}
    spread = lambda r: {k: (max(v) - min(v)) / float(np.median(v)) for k, v in r["all"].items()}
    return dict(envs=n, rows=n * steps, backward_us=us(back), backward_window_spread=spread(back), backward_calls_per_s_all=back["all"],
                rollout_us=us(roll), rollout_window_spread=spread(roll), rollouts_per_s_all=roll["all"])


def main_distill(args):
    """--distill [--beta B --beta-decay D --iters K] [out.json]: the learning run at 512 envs and the timings at 4096 and 512, a process
    per case; results to profiles/policy_imitation.json"""
    import subprocess
    opts = dict(beta=1.0, decay=0.8, iters=20)
    rest = []
    while args:
        a = args.pop(0)
        if a in ("--beta", "--beta-decay", "--iters"):
            opts[dict({"--beta": "beta", "--beta-decay": "decay", "--iters": "iters"})[a]] = float(args.pop(0))
        else:
            rest.append(a)
    if rest and rest[0] == "--trace":                 # backward() with the term off, then on, for rocprofv3 --kernel-trace --stats
        from tsid_control_amd import PolicyLearner, RolloutStorage
        n, calls = int(rest[1]), int(rest[2])
        env = distill_env(n)
        pa = distill_actor(env)
        st = env.rollout(pa, 16, RolloutStorage(env, pa, 16, teacher=True), teacher_beta=0.5)
        st.gae(0.99, 0.95)
        index = torch.randperm(n * 16, dtype=torch.int32, device="cuda:0")
        for kw in (dict(), dict(imitation_coef=0.5)):
            pl = PolicyLearner(pa, entropy_coef=0.01, **kw)
            for _ in range(calls):
                pl.backward(st, index)
        torch.cuda.synchronize()
        return
    if rest and rest[0] == "--case":                  # one case, as a JSON line
        what, n = rest[1], int(rest[2])
        if what == "time":
            print(json.dumps(time_distill(n)))
        else:
            print(json.dumps(run_distill(n, opts["beta"], opts["decay"], int(opts["iters"])) if what == "run" else
                             run_distill(n, 0.0, 1.0, int(opts["iters"]), learn=False)))
        return
    out_path = rest[0] if rest else "profiles/policy_imitation.json"
    flags = ["--beta", str(opts["beta"]), "--beta-decay", str(opts["decay"]), "--iters", str(int(opts["iters"]))]
    case = lambda *c: json.loads(subprocess.run([sys.executable, sys.argv[0], "--distill", *flags, "--case", *c], capture_output=True, text=True,
                                                check=True).stdout.strip().splitlines()[-1])
    report(out_path, actor="obs -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU (not trained: pure distillation)",
           env="tsid = 'stand', motor mode, action = torque [N m], decimation 4", optimizer="PolicyOptimizer, lr 1e-3, max_grad_norm 1",
           run=case("run", "512"), control=case("control", "512"), timings=[case("time", "4096"), case("time", "512")])


EP_TERRAIN = dict(TERRAIN, num_levels=3)
EP_CURRICULUM = dict(up_distance=0.05, down_fraction=0.5, random_top=True)


class TorchEpisodes:
    """the slice's bookkeeping with torch ops after each step() of a plain env, as a caller had to write it: running sums of
    reward and terms, records of the finished episodes, legged_gym's level rule.  It runs behind the reset, so the position it
    reads for a done env is already the new episode's: its displacement of a finished episode is wrong (measured from the
    penultimate position here), and its level reaches the terrain one episode late.  The cost is what is compared."""

    def __init__(self, env, cur):
        self.env, self.cur = env, cur
        n, dev = env.num_envs, env.device
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        self.run, self.last, self.sum, self.start = z(n, _lib.POL_EP_NREC), z(n, _lib.POL_EP_NREC), z(n, _lib.POL_EP_NREC), env.wc.qpos[:, :2].double().clone()
        self.prev_xy, self.prev_cmd = env.wc.qpos[:, :2].double().clone(), env.command[:, :2].double().clone()
        self.t_episode = float(env.params[_lib.POL_P_MAX_EPISODE_STEPS]) * env.decimation * env.wc.conf.dt
        self.levels = int(env.ter_params[_lib.POL_TER_NUM_LEVELS])

    def step(self, action):
        env = self.env
        _, reward, done, info = env.step(action)
        fin = lambda x: torch.where(torch.isfinite(x), x, torch.zeros_like(x)).double()
        self.run[:, _lib.POL_EP_LENGTH] += 1
        self.run[:, _lib.POL_EP_RETURN] += fin(reward)
        self.run[:, _lib.POL_EP_TERMS:_lib.POL_EP_TEACH] += fin(info["terms"])
        fresh = done != 0
        d = (self.prev_xy - self.start).norm(dim=1)
        lvl = env.terrain_level.clamp(0, self.levels - 1)
        rec = self.run.clone()
        rec[:, _lib.POL_EP_COUNT], rec[:, _lib.POL_EP_TIMEOUT], rec[:, _lib.POL_EP_DISPLACEMENT] = 1, info["timeout"].double(), d
        rec[:, _lib.POL_EP_LEVEL] = lvl.double()
        self.last = torch.where(fresh[:, None], rec, self.last)
        self.sum += torch.where(fresh[:, None], torch.nan_to_num(rec), torch.zeros_like(rec))
        up = d > self.cur["up_distance"]
        down = (d < self.prev_cmd.norm(dim=1) * self.t_episode * self.cur["down_fraction"]) & ~up
        new = lvl + up.int() - down.int()
        new = torch.where(new >= self.levels, torch.randint_like(new, self.levels), new.clamp(min=0))
        env.terrain_level.copy_(torch.where(fresh, new, env.terrain_level))
        xy = env.wc.qpos[:, :2].double()
        self.start = torch.where(fresh[:, None], xy, self.start)
        self.run *= (~fresh)[:, None]
        self.prev_xy.copy_(xy)
        self.prev_cmd.copy_(env.command[:, :2])


def measure_episodes(n, decimation, window=300, windows=4, preroll=60):
    """off: PolicyEnv(terrain=EP_TERRAIN); on: the same with the curriculum (statistics and levels on the device); torch: `off`
    with TorchEpisodes behind every step.  Policy-steps/s in alternating windows of one process"""
    delay = delays(n)
    make = lambda **kw: PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, terrain=EP_TERRAIN, **kw, **KW)
    envs = dict(off=make(), on=make(curriculum=EP_CURRICULUM), torch=make())
    book = TorchEpisodes(envs["torch"], EP_CURRICULUM)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    actions = [(torch.rand(n, envs["on"].NA, generator=g, dtype=torch.float64, device="cuda:0") - 0.5) * 0.2 for _ in range(16)]
    run = {k: stepper(envs[k], n, envs[k].NA) for k in ("off", "on")}
    run["torch"] = lambda k: [book.step(actions[i & 15]) for i in range(k)]
    r = alternate(run, window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    stats = {k: float(v) for k, v in envs["on"].episode_stats().items()}
    return dict(envs=n, decimation=decimation, window_policy_steps=window, windows=windows, **r, on_over_off=med["on"] / med["off"],
                torch_over_off=med["torch"] / med["off"], episode_us_per_policy_step=us["on"] - us["off"],
                torch_us_per_policy_step=us["torch"] - us["off"], torch_cost_over_fused_cost=(us["torch"] - us["off"]) / max(us["on"] - us["off"], 1e-9),
                restarts={k: int(e.episode.sum()) - n for k, e in envs.items()}, episode_stats_on=stats)


def curriculum_run(n=512, iters=10, levels=8, height=0.04, up_distance=None, steps=400, decimation=4):
    """TSID walking with a zero residual on stepped terrain with the curriculum on: per iteration (one episode length of policy
    steps) the level histogram and the episode statistics; per level the share of its finished episodes that went up"""
    from tsid_control_amd.walk_planner import op3_closed_loop_walking_conf
    conf = op3_closed_loop_walking_conf(RobotConfig())
    conf.closed_loop, conf.reference_quirks = True, False
    ter = dict(seed=1, step_height=(height, height), step_length=(0.03, 0.06), step_prob=0.5, flat_cells=0, num_levels=levels)   # (short strips, none kept flat but the one under the robot: a 3.2 s walk of some 12 cm crosses several edges)
    kw = dict(num_envs=n, device="cuda:0", decimation=decimation, mode="residual", action_scale=0.05, max_episode_steps=steps, tsid="walk",
              teacher_weights=TEACH, reward_weights=WEIGHTS, terrain=ter, command_range=((0.08, 0.08), (0.0, 0.0), (0.0, 0.0)))   # (about TSID's own pace: less than half of it moves an env down)
    if up_distance is None:        # half of what TSID walks in an episode on the level floor, measured first
        flat = PolicyEnv(conf, episode_stats=True, **dict(kw, terrain=dict(ter, step_height=(0.0, 0.0))))
        a = torch.zeros(n, flat.NA, dtype=flat.dtype, device=flat.device)
        for _ in range(steps):
            flat.step(a)
        s = flat.episode_stats()
        flat_stats = {k: float(s[k]) for k in ("episodes", "timeouts", "length", "displacement")}
        up_distance = 0.5 * flat_stats["displacement"]
    else:
        flat_stats = None
    env = PolicyEnv(conf, curriculum=dict(up_distance=up_distance, down_fraction=0.5, random_top=False), **kw)
    a = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
    out, ups, ends = [], torch.zeros(levels, device=env.device), torch.zeros(levels, device=env.device)
    for it in range(iters):
        for _ in range(steps):
            _, _, done, info = env.step(a)
            rec = info["episode_last"]
            fresh = done != 0
            lvl = rec[:, _lib.POL_EP_LEVEL].long()
            ends.index_add_(0, lvl, fresh.float())
            ups.index_add_(0, lvl, (fresh & (rec[:, _lib.POL_EP_DISPLACEMENT] > up_distance)).float())
        s = env.episode_stats()
        out.append(dict(iteration=it, level_histogram=torch.bincount(env.terrain_level.long(), minlength=levels).tolist(),
                        **{k: float(s[k]) for k in ("episodes", "timeouts", "length", "return", "displacement", "level")}))
    share = (ups / ends.clamp(min=1)).tolist()
    return dict(envs=n, tsid="walk", mode="residual, zero residual", policy_steps_per_iteration=steps, decimation=decimation, num_levels=levels,
                step_height_of_level_m=[height * (l + 1) / levels for l in range(levels)], up_distance_m=up_distance, flat_floor=flat_stats,
                iterations=out, episodes_finished_by_level=ends.tolist(), share_that_went_up_by_level=share)


def main_episodes(args):
    """--episodes: the cost of the slice against off and against torch bookkeeping, and the curriculum under TSID's walk"""
    if args and args[0] == "--trace":
        n, k = int(args[1]), int(args[2])
        env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=4, terrain=EP_TERRAIN, curriculum=EP_CURRICULUM, **KW)
        a = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
        for _ in range(k):
            env.step(a)
        torch.cuda.synchronize()
        return
    if args and args[0] == "--curriculum":
        print(json.dumps(curriculum_run(), indent=1))
        return
    out_path = args[0] if args else "profiles/policy_episode.json"
    report(out_path, terrain=EP_TERRAIN, curriculum=EP_CURRICULUM, runs=[measure_episodes(n, 4) for n in (4096, 512)],
           curriculum_under_tsid_walk=curriculum_run())


class TorchHistory:
    """the observation history with torch ops behind every step: a cat, a where on done, a repeat for the restarted envs"""

    def __init__(self, env, frames):
        self.env, self.frames = env, frames
        self.hist = env.obs.repeat(1, frames)

    def step(self, action):
        obs, _, done, _ = self.env.step(action)
        pushed = torch.cat([self.hist[:, obs.shape[1]:], obs], 1)
        self.hist = torch.where((done != 0)[:, None], obs.repeat(1, self.frames), pushed)


def history_bytes(n, K, frames, item=8):
    """what one tsidb_policy_obs_history launch moves when no env restarts: frames - 1 frames read and written, the current
    selection read, the newest frame written"""
    return n * K * item * (2 * (frames - 1) + 2)


def measure_history(n, frames, decimation=4, window=300, windows=4, preroll=60, rollout_steps=16):
    """off: PolicyEnv; on: the same with obs_history on obs; torch: `off` with TorchHistory behind every step.  Policy-steps/s in
    alternating windows of one process; then rollouts of an actor that reads the stacked row"""
    from tsid_control_amd import PolicyActor
    delay = delays(n)
    make = lambda **kw: PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=decimation, delay=delay, **kw, **KW)
    envs = dict(off=make(), on=make(obs_history=dict(frames=frames, sources=("obs",))), torch=make())
    book = TorchHistory(envs["torch"], frames)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    actions = [(torch.rand(n, envs["on"].NA, generator=g, dtype=torch.float64, device="cuda:0") - 0.5) * 0.2 for _ in range(16)]
    run = {k: stepper(envs[k], n, envs[k].NA) for k in ("off", "on")}
    run["torch"] = lambda k: [book.step(actions[i & 15]) for i in range(k)]
    r = alternate(run, window, windows, preroll)
    med, us = r["policy_steps_per_s_median"], r["us_per_policy_step"]
    K = envs["on"].NOBS
    out = dict(envs=n, decimation=decimation, frames=frames, K=K, window_policy_steps=window, windows=windows, **r,
               on_over_off=med["on"] / med["off"], torch_over_off=med["torch"] / med["off"], history_us_per_policy_step=us["on"] - us["off"],
               torch_us_per_policy_step=us["torch"] - us["off"], torch_cost_over_fused_cost=(us["torch"] - us["off"]) / max(us["on"] - us["off"], 1e-9),
               torch_history_equals_fused=bool(torch.equal(book.hist, envs["on"].obs_history)),   # (the same actions, the same number of steps)
               bytes_per_launch_without_restarts=history_bytes(n, K, frames), restarts={k: int(e.episode.sum()) - n for k, e in envs.items()})
    env = envs["on"]
    if frames * K > _lib.POL_NET_MAXWIDTH:
        out["actor_rollout"] = f"not run: frames * K = {frames * K} columns exceed the actor's {_lib.POL_NET_MAXWIDTH}"
        return out
    torch.manual_seed(1)
    mlp = lambda k, last: torch.nn.Sequential(torch.nn.Linear(k, 256), torch.nn.ELU(), torch.nn.Linear(256, 128), torch.nn.ELU(),
                                              torch.nn.Linear(128, last)).to("cuda:0")
    both = {}
    for name, e, inputs in (("obs", envs["off"], ("obs",)), ("obs_history", env, ("obs_history",))):
        k_in = e.NOBS if name == "obs" else frames * K
        with torch.no_grad():
            actor = mlp(k_in, e.NA)
            actor[-1].weight.mul_(0.05)                       # (small actions: the robots keep standing)
        pa = PolicyActor(e, actor, mlp(e.NOBS + 4, 1), actor_inputs=inputs, critic_inputs=("obs", "priv"),
                         log_std=torch.full((e.NA,), -3.0, device="cuda:0"))
        st = e.rollout(pa, rollout_steps)
        both[name] = (lambda e, pa, st: lambda k: [e.rollout(pa, rollout_steps, st) for _ in range(k)])(e, pa, st)
    rr = alternate(both, 10, windows, 3, per_call=rollout_steps)
    out["actor_rollout"] = dict(actor=f"{frames * K} -> 256 -> 128 -> NA against {K} -> 256 -> 128 -> NA, ELU; eager {rollout_steps}-step rollouts", **rr)
    return out


def main_history(args):
    """--history H: the cost of the history against off and against the torch stack, and an actor rollout on the stacked row"""
    frames, args = int(args[0]), args[1:]
    if args and args[0] == "--trace":
        n, k = int(args[1]), int(args[2])
        env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=4, obs_history=dict(frames=frames, sources=("obs",)), **KW)
        a = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
        for _ in range(k):
            env.step(a)
        torch.cuda.synchronize()
        print(json.dumps(dict(envs=n, steps=k, frames=frames, K=env.NOBS, bytes_per_launch_without_restarts=history_bytes(n, env.NOBS, frames))))
        return
    out_path = args[0] if args else "profiles/policy_obs_history.json"
    report(out_path, obs_history=dict(frames=frames, sources=["obs"]), runs=[measure_history(n, frames) for n in (4096, 512)])


class TorchSymmetryLearner(TorchLearner):
    """TorchLearner with rsl_rl's symmetry in eager torch: the minibatch gathered, mirrored and concatenated into one batch of 2 M
    rows for the surrogate and the value loss (augment), and the mirror loss against the detached, mirrored mean"""

    def __init__(self, sym, augment, mirror_coef, *a, **kw):
        super().__init__(*a, **kw)
        self.augment, self.mirror_coef = augment, mirror_coef
        tables = dict(actor=(sym.actor_perm, sym.actor_sign), critic=(sym.critic_perm, sym.critic_sign), action=(sym.action_perm, sym.action_sign))
        self.tables = {k: (p.long(), s) for k, (p, s) in tables.items()}     # (int64 once: torch's index wants it)

    def mirror(self, x, which):
        perm, sign = self.tables[which]
        return x[:, perm] * sign

    def loss(self, st, index):
        rows, c, ls = st.logp.numel(), self.clip, self.log_std
        j = index.long()
        m = j.shape[0]
        flat = lambda t: t.reshape(rows, -1)[j]
        x, xc, a = flat(st.actor_input), flat(st.critic_input), flat(st.action)
        mu_all = self.actor(torch.cat([x, self.mirror(x, "actor")]))
        n = 2 * m if self.augment else m
        rep = (lambda t: torch.cat([t, t])) if self.augment else (lambda t: t)
        v = self.critic(torch.cat([xc, self.mirror(xc, "critic")])[:n]).squeeze(1)
        z = (torch.cat([a, self.mirror(a, "action")])[:n] - mu_all[:n]) / ls.exp()
        logp = -(0.5 * z * z + ls).sum(1) - 0.5 * a.shape[1] * 1.8378770664093453
        r = (logp - rep(st.logp.reshape(-1)[j])).exp()
        adv = rep((st.advantage.reshape(-1)[j] - self.adv_stats[0]) * self.adv_stats[1])
        l_pi = torch.max(-adv * r, -adv * r.clamp(1 - c, 1 + c)).mean()
        old, ret = rep(st.value[:-1].reshape(-1)[j]), rep(st.returns.reshape(-1)[j])
        l_v = torch.max((v - ret) ** 2, (old + (v - old).clamp(-c, c) - ret) ** 2).mean()
        entropy = (ls + 0.5 * (1 + 1.8378770664093453)).sum()
        self.l_sym = ((mu_all[m:] - self.mirror(mu_all[:m].detach(), "action")) ** 2).mean()
        return l_pi + self.value_coef * l_v - self.entropy_coef * entropy + self.mirror_coef * self.l_sym


def measure_symmetry(n, minibatches=4, window=40, windows=4, preroll=3, mirror_coef=0.5):
    """backward() calls/s on one minibatch of a recorded rollout, in alternating windows of one process: the plain learner; the
    learner with a symmetry - augmentation alone, the mirror term alone, both; and the loss of `both` in eager torch with
    autograd.  Also the first minibatch's loss and L_sym from the fused and the torch learner before either has moved a weight."""
    from tsid_control_amd import PolicyLearner, PolicySymmetry
    st, plain, copies = learn_setup(n)
    pa = plain.actor
    sy = PolicySymmetry(pa.env, pa)
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01)
    fused = {name: PolicyLearner(pa, symmetry=sy, symmetry_augment=aug, mirror_coef=coef, **kw)
             for name, aug, coef in (("augment", True, 0.0), ("mirror", False, mirror_coef), ("both", True, mirror_coef))}
    eager = TorchSymmetryLearner(sy, True, mirror_coef, copies.actor, copies.critic, pa.log_std.detach(), **kw)
    rows = st.logp.numel()
    index = torch.randperm(rows, generator=torch.Generator(device="cuda:0").manual_seed(3), dtype=torch.int32, device="cuda:0")[:rows // minibatches].contiguous()
    plain.fill_adv_stats(st)
    eager.adv_stats = plain.adv_stats.clone()
    for pl in fused.values():
        pl.adv_stats.copy_(plain.adv_stats)
    stats = fused["both"].backward(st, index, adv_stats=fused["both"].adv_stats).clone()
    grad_torch = torch.autograd.grad(eager.loss(st, index), eager.parameters())
    grad_rel = max(float((a.grad - b).abs().max() / b.abs().max()) for a, b in zip(fused["both"].parameters(), grad_torch))
    with torch.no_grad():
        loss_torch = float(eager.loss(st, index))

    def torch_backward(k):
        for _ in range(k):
            for p in eager.parameters():
                p.grad = None
            eager.loss(st, index).backward()
    run = dict(plain=lambda k: [plain.backward(st, index, adv_stats=plain.adv_stats) for _ in range(k)], torch_both=torch_backward)
    for name, pl in fused.items():
        run[name] = lambda k, pl=pl: [pl.backward(st, index, adv_stats=pl.adv_stats) for _ in range(k)]
    r = alternate(run, window, windows, preroll)
    med = r["policy_steps_per_s_median"]
    return dict(envs=n, rollout_steps=st.steps, rows=rows, minibatch_rows=int(index.shape[0]), mirror_coef=mirror_coef, window_calls=window, windows=windows,
                backward_per_s_median=med, backward_per_s_all=r["all"], us_per_backward={k: 1e6 / v for k, v in med.items()},
                over_plain={k: med["plain"] / med[k] for k in fused}, both_over_torch=med["both"] / med["torch_both"],
                first_minibatch=dict(loss_fused=float(stats[5]), loss_torch=loss_torch, mirror_loss_fused=float(fused["both"].sym_stats[0]),
                                     mirror_loss_torch=float(eager.l_sym), largest_gradient_difference_over_largest_entry=grad_rel,
                                     rows_used=float(stats[6]), mirrored_rows=float(fused["both"].sym_stats[1])))


def main_symmetry(args):
    """--symmetry: backward() with augmentation and with the mirror term against the plain backward() and against eager torch, at
    4096 x 16 and 512 x 16 rows with the 256-128 networks; a process per case"""
    import subprocess
    if args and args[0] == "--case":
        print(json.dumps(measure_symmetry(int(args[1]))))
        return
    out_path = args[0] if args else "profiles/policy_symmetry.json"
    runs = []
    for n in (4096, 512):
        r = subprocess.run([sys.executable, sys.argv[0], "--symmetry", "--case", str(n)], capture_output=True, text=True, check=True)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    report(out_path, actor="obs -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU",
           loss="clip 0.2, value_coef 1, entropy_coef 0.01, clipped value loss, normalised advantages; mirror_coef 0.5",
           tables="derived from the model blob: obs and obs | priv of the v1 robot, mirror normal x", runs=runs)


def main_normalize(which, args):
    """--actor --normalize / --learn --normalize: the section's method (a process per case, four alternating windows, medians,
    4096 and 512 envs) with the normaliser on; each run replaces its own entry of profiles/policy_norm.json"""
    import os
    import subprocess
    from tsid_control_amd import PolicyActor, PolicyNormalizer
    if args and args[0] == "--trace":
        n, k = int(args[1]), int(args[2])
        if which == "actor":                  # the normaliser off, then on: k_policy_actor beside k_policy_actor_norm and the update's two
            env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=4, **dict(KW, action_scale=0.05))
            for nz in (None, PolicyNormalizer()):
                actor, critic, ai, ci, ls = actor_nets(env, False)
                env.rollout(PolicyActor(env, actor, critic, actor_inputs=ai, critic_inputs=ci, log_std=ls, normalizer=nz), k).gae(0.99, 0.95)
        else:
            st, fused, _ = learn_setup(n, normalize=True)
            opt = torch.optim.Adam(fused.parameters(), lr=1e-4)
            for _ in range(k):
                fused.update(st, opt, 5, 4)
        torch.cuda.synchronize()
        return
    if args and args[0] == "--case":
        n = int(args[1])
        print(json.dumps(measure_actor(n, False, normalize=True) if which == "actor" else measure_learn(n, normalize=True)))
        return
    out_path = args[0] if args else "profiles/policy_norm.json"
    runs = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            runs = json.load(f).get("runs", {})
    runs[which] = []
    for n in (4096, 512):
        r = subprocess.run([sys.executable, sys.argv[0], "--" + which, "--normalize", "--case", str(n)], capture_output=True, text=True, check=True)
        runs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    report(out_path, actor="obs -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU", normalizer="eps 1e-2, no clip, both networks",
           runs=runs)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--history":
        main_history(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--symmetry":
        main_symmetry(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--episodes":
        main_episodes(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--distill":
        main_distill(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] in ("--actor", "--learn") and sys.argv[2] == "--normalize":
        main_normalize(sys.argv[1][2:], sys.argv[3:])
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "--learn" and sys.argv[2] == "--optimizer":
        main_optimizer(sys.argv[3:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--learn":
        if len(sys.argv) > 2 and sys.argv[2] == "--trace":
            st, fused, _ = learn_setup(int(sys.argv[3]))
            opt = torch.optim.Adam(fused.parameters(), lr=1e-4)
            for _ in range(int(sys.argv[4])):
                fused.update(st, opt, 5, 4)
            torch.cuda.synchronize()
            sys.exit(0)
        if len(sys.argv) > 2 and sys.argv[2] == "--case":           # one env count, as a JSON line
            print(json.dumps(measure_learn(int(sys.argv[3]))))
            sys.exit(0)
        import subprocess
        out_path = sys.argv[2] if len(sys.argv) > 2 else "profiles/policy_learner.json"
        runs = []
        for n in (4096, 512):
            r = subprocess.run([sys.executable, sys.argv[0], "--learn", "--case", str(n)], capture_output=True, text=True, check=True)
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        report(out_path, actor="obs -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU", optimizer="Adam, lr 1e-4",
               loss="clip 0.2, value_coef 1, entropy_coef 0.01, clipped value loss, normalised advantages", runs=runs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--actor":
        from tsid_control_amd import PolicyActor
        if len(sys.argv) > 2 and sys.argv[2] == "--trace":
            n, k = int(sys.argv[3]), int(sys.argv[4])
            env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=4, terrain=TERRAIN, **dict(KW, action_scale=0.05))
            for scan in (False, True):
                actor, critic, ai, ci, ls = actor_nets(env, scan)
                env.rollout(PolicyActor(env, actor, critic, actor_inputs=ai, critic_inputs=ci, log_std=ls), k).gae(0.99, 0.95)
            torch.cuda.synchronize()
            sys.exit(0)
        if len(sys.argv) > 2 and sys.argv[2] == "--case":           # one (envs, actor input) case, as a JSON line
            print(json.dumps(measure_actor(int(sys.argv[3]), sys.argv[4] == "scan")))
            sys.exit(0)
        import subprocess
        out_path = sys.argv[2] if len(sys.argv) > 2 else "profiles/policy_actor.json"
        runs = []
        for n in (4096, 512):                                       # a process per case: four envs and two captured graphs each
            for scan in ("obs", "scan"):
                r = subprocess.run([sys.executable, sys.argv[0], "--actor", "--case", str(n), scan], capture_output=True, text=True, check=True)
                runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        report(out_path, actor="K -> 256 -> 128 -> NA, ELU", critic="obs | priv -> 256 -> 128 -> 1, ELU", runs=runs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--tsid":
        import os
        tsid, rest = sys.argv[2], sys.argv[3:]
        mode = "residual"
        if rest and rest[0] == "--mode":
            mode, rest = rest[1], rest[2:]
        out_path = rest[0] if rest else "profiles/policy_tsid.json"
        runs = {}
        if os.path.exists(out_path):
            with open(out_path) as f:
                runs = json.load(f).get("runs", {})
        runs[f"{tsid}/{mode}"] = [measure_tsid(n, tsid, mode) for n in (4096, 512)]
        report(out_path, runs=runs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--terrain":
        if len(sys.argv) > 2 and sys.argv[2] == "--trace":
            n, k = int(sys.argv[3]), int(sys.argv[4])
            env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=4, terrain=TERRAIN, **KW)
            a = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
            for _ in range(k):
                env.step(a)
            torch.cuda.synchronize()
            sys.exit(0)
        out_path = sys.argv[2] if len(sys.argv) > 2 else "profiles/policy_terrain.json"
        report(out_path, terrain=TERRAIN, runs=[measure_terrain(n, d) for n in (4096, 512) for d in (4, 10)])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--randomize":
        out_path = sys.argv[2] if len(sys.argv) > 2 else "profiles/policy_dr.json"
        report(out_path, randomization=RANDOMIZATION, runs=[measure_randomize(n, d) for n in (4096, 512) for d in (4, 10)])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n, k = int(sys.argv[2]), int(sys.argv[3])
        env = PolicyEnv(RobotConfig(), num_envs=n, device="cuda:0", decimation=10, **KW)
        a = torch.zeros(n, env.NA, dtype=env.dtype, device=env.device)
        for _ in range(k):
            env.step(a)
        torch.cuda.synchronize()
        sys.exit(0)
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/policy_env.json"
    report(out_path, runs=[measure(n, d) for n in (4096, 512) for d in (4, 10)])
