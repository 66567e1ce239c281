"""PolicyEnv - the environment a learned policy steps: actions in, observations, rewards and done flags out, everything on the
device.  No reference counterpart (the reference's only controller is TSID, main.py:113-129); it stands on the sim stage's
direct actuator control (WalkController.set_ctrl / sim_steps) and adds what a policy loop needs around it as three HIP
kernels (include/tsidb.h tsidb_policy_act / _reward / _obs; csrc/tsidb_policy.hpp).

One step() is, on the current stream and without a host round trip:
    act      clip, delay, scale and filter the action into the ctrl buffer
    sim      `decimation` sim steps with ctrl held (tsidb_sim_ctrl, up to 8 steps per launch)
    reward   reward terms, termination / timeout -> reward and done in the controller's rows
    reset    tsidb_reset_done restarts exactly the done envs
    obs      bookkeeping of the restarted envs, then the observation row of every env
With a PolicyRandomization two more launches join them, each only while its group is on - the push of this step into the torso
force before the sim steps (tsidb_policy_perturb), noise on the state of the envs just reset before the observation
(tsidb_policy_reset_noise) - and the obs launch resamples commands and adds observation noise.  Every draw is a hash of
(seed, stream, column, env, episode, ep_len): no random state, so a captured step replays and a split batch draws alike.
"""
import copy
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .walk_controller import WalkController, _ptr


@dataclasses.dataclass
class PolicyRandomization:
    """Per-episode and per-step randomisation of a PolicyEnv (include/tsidb.h TSIDB_POL_DR_*); every value defaults to 0 = off.
    seed: of all draws but the command components', which keep the env's seed (None = the env's seed; below 2^32).  env_offset:
    added to the env index in every draw - a batch split over ranks passes each rank's first env and draws what the unsplit
    batch draws.  Reset noise, uniform in +-amplitude, on the envs a step or reset() restarts: reset_joint_pos [rad],
    reset_joint_vel [rad/s], reset_base_lin_vel [m/s, world; a scalar or (x, y, z)], reset_base_ang_vel [rad/s; same],
    reset_yaw [rad, about world z], reset_xy [m]; reset_lift [m] is added to the base height as it is.  Observation noise,
    uniform in +-amplitude, on the observation columns only: noise_ang_vel, noise_gravity, noise_joint_pos, noise_joint_vel.
    Pushes: every push_interval policy steps (at a per-episode phase) a horizontal force of push_force_lo .. push_force_hi [N]
    in a random direction acts on the torso for push_duration policy steps.  Commands: redrawn every command_interval policy
    steps (0 = at restarts only); at a restart or a redraw all three are 0 with probability command_zero_prob."""
    seed: int = None
    env_offset: int = 0
    reset_joint_pos: float = 0.0
    reset_joint_vel: float = 0.0
    reset_base_lin_vel: object = 0.0
    reset_base_ang_vel: object = 0.0
    reset_yaw: float = 0.0
    reset_xy: float = 0.0
    reset_lift: float = 0.0
    noise_ang_vel: float = 0.0
    noise_gravity: float = 0.0
    noise_joint_pos: float = 0.0
    noise_joint_vel: float = 0.0
    push_interval: int = 0
    push_duration: int = 0
    push_force_lo: float = 0.0
    push_force_hi: float = 0.0
    command_interval: int = 0
    command_zero_prob: float = 0.0

    @classmethod
    def of(cls, r):
        """r as a PolicyRandomization: one, or a dict of its fields"""
        if isinstance(r, cls):
            return r
        if not isinstance(r, dict):
            raise _lib.TsidbError(f"PolicyEnv: randomization must be a PolicyRandomization or a dict, got {type(r).__name__}")
        unknown = sorted(set(r) - set(_lib.POL_DR_FIELDS))
        if unknown:
            raise _lib.TsidbError(f"PolicyEnv: unknown randomization fields {unknown} (known: {_lib.POL_DR_FIELDS})")
        return cls(**r)

    def params(self, default_seed=0):
        """the float64 vector tsidb_policy_randomize takes, checked as the library checks it"""
        p = np.zeros(_lib.POL_DR_NPARAMS)
        for k in _lib.POL_DR_FIELDS:
            v = getattr(self, k)
            if k == "seed" and v is None:
                v = default_seed
            i = getattr(_lib, "POL_DR_" + k.upper())
            try:
                if k in ("reset_base_lin_vel", "reset_base_ang_vel"):
                    p[i:i + 3] = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
                else:
                    p[i] = float(v)
            except (TypeError, ValueError) as err:
                raise _lib.TsidbError(f"PolicyRandomization: {k} = {v!r} is not a number{' or three' if i in (4, 7) else ''}") from err
        bad = lambda msg: _lib.TsidbError("PolicyRandomization: " + msg)
        if not np.isfinite(p).all():
            raise bad("non-finite value")
        if (p < 0).any():
            raise bad("negative value: amplitudes, forces, intervals, seed, offset and probability are all >= 0")
        for k in ("seed", "env_offset", "push_interval", "push_duration", "command_interval"):
            i = getattr(_lib, "POL_DR_" + k.upper())
            if p[i] != math.floor(p[i]) or p[i] >= 2.0 ** (32 if k == "seed" else 31):
                raise bad(f"{k} must be a whole number below 2^{32 if k == 'seed' else 31}, got {p[i]}")
        if p[_lib.POL_DR_PUSH_DURATION] > p[_lib.POL_DR_PUSH_INTERVAL]:
            raise bad("push_duration > push_interval")
        if p[_lib.POL_DR_PUSH_FORCE_LO] > p[_lib.POL_DR_PUSH_FORCE_HI]:
            raise bad("push_force_lo > push_force_hi")
        if p[_lib.POL_DR_COMMAND_ZERO_PROB] > 1:
            raise bad("command_zero_prob must be in [0, 1]")
        return p


class PolicyEnv:
    """conf: a RobotConfig (used as a copy with reference_quirks = False, sim_enabled = True: a reset then writes a proper wxyz
    qpos).  decimation: sim steps per policy step.  mode: "position" (ctrl = joint targets [rad] = default_joint_pos +
    action_scale * action) or "motor" (torques [N m]; default_joint_pos is then an offset torque, normally 0).  action_scale,
    default_joint_pos: scalars or [NA] in the actuator order (default pose None = the standing joints in position mode, 0 in
    motor mode).  action_clip: actions are clipped to +-action_clip.  delay: [N] int32 tensor of actuation delays in policy steps
    (0 .. 7) used in place, or None.  filter_alpha in (0, 1]: ctrl += alpha (target - ctrl).  command_range: ((lo, hi),) * 3 for
    vx, vy, yaw rate - a restart redraws the components with lo != hi, the others keep what the caller wrote into
    self.command.  max_episode_steps: policy steps until the timeout (0 = none).  reward_weights: {term: weight} over
    _lib.POL_TERMS, missing terms weigh 0.  term_bodies: sim bodies whose floor contact ends the episode (None = the torso).
    sigma, h_target (None = the standing height), t_air, deadband, seed: the reward's constants.  randomization: a
    PolicyRandomization or a dict of its fields (None = none); with pushes on, an xfrc buffer is registered (wc.set_xfrc) unless
    the caller has registered one, and info["push"] is the view xfrc[:, 0, :3] of the torso force of the step.

    Tensors, all used in place: obs [N, NOBS], priv [N, 4] (base linear velocity in the body frame, base height), reward [N],
    done [N] (views of wc.rows), command [N, 3], delay [N], terms [N, 12], timeout [N], ep_len [N], episode [N], last_action,
    prev_action [N, NA], air_time [N, 2], act_hist [8, N, NA]; wc is the WalkController underneath."""

    # the randomisation's launches a step makes; class-level so that an instance built without __init__ steps unrandomised
    randomization = None
    _dr_push = _dr_reset = False

    def __init__(self, conf=None, num_envs=None, device=None, decimation=10, mode="position", action_scale=0.25,
                 default_joint_pos=None, action_clip=100.0, delay=None, filter_alpha=1.0, command_range=((0.0, 0.0),) * 3,
                 max_episode_steps=0, reward_weights=None, term_bodies=None, sigma=0.25, h_target=None, t_air=0.25, deadband=0.1,
                 seed=0, randomization=None):
        from .conf import RobotConfig
        conf = copy.copy(conf) if conf is not None else RobotConfig()
        conf.reference_quirks = False
        conf.sim_enabled = True
        if mode not in ("position", "motor"):
            raise _lib.TsidbError(f"PolicyEnv: mode must be 'position' or 'motor', got {mode!r}")
        dr = None
        if randomization is not None:
            self.randomization = PolicyRandomization.of(randomization)
            dr = self.randomization.params(seed)      # (checked before anything is built)
        self.wc = wc = WalkController(conf, num_envs=num_envs, device=device)
        self.num_envs, self.device, self.dtype, self.NA = wc.num_envs, wc.device, wc.dtype, wc.NA
        N, NA = wc.num_envs, wc.NA
        self.NOBS = _lib.pol_nobs(NA)
        self.decimation, self.mode = int(decimation), mode
        z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
        wc.set_ctrl(z(N, NA), mode)
        weights = dict(reward_weights or {})
        unknown = sorted(set(weights) - set(_lib.POL_TERMS))
        if unknown:
            raise _lib.TsidbError(f"PolicyEnv: unknown reward terms {unknown} (known: {_lib.POL_TERMS})")
        if weights.get("torques", 0.0) != 0.0:     # the readout kernels cost 3-4 %: only when the term is used
            wc.enable_sim_readouts()
        if default_joint_pos is None:
            default_joint_pos = wc.ctrl_from_q(wc.q0)[0].double().cpu().numpy() if mode == "position" else 0.0
        self.action_scale = np.broadcast_to(np.asarray(action_scale, dtype=np.float64), (NA,)).copy()
        self.default_joint_pos = np.broadcast_to(np.asarray(default_joint_pos, dtype=np.float64), (NA,)).copy()
        self.term_body_mask = 1 if term_bodies is None else sum(1 << int(b) for b in set(term_bodies))
        p = np.zeros(_lib.POL_NPARAMS)
        p[_lib.POL_P_CLIP], p[_lib.POL_P_ALPHA], p[_lib.POL_P_SIGMA] = action_clip, filter_alpha, sigma
        p[_lib.POL_P_H_TARGET] = float(wc.qpos[0, 2]) if h_target is None else h_target
        p[_lib.POL_P_T_AIR], p[_lib.POL_P_DEADBAND] = t_air, deadband
        p[_lib.POL_P_MAX_EPISODE_STEPS], p[_lib.POL_P_DECIMATION], p[_lib.POL_P_SEED] = max_episode_steps, self.decimation, seed
        rng = np.asarray(command_range, dtype=np.float64).reshape(3, 2)
        p[_lib.POL_P_CMD_LO:_lib.POL_P_CMD_LO + 3], p[_lib.POL_P_CMD_HI:_lib.POL_P_CMD_HI + 3] = rng[:, 0], rng[:, 1]
        for k, w in weights.items():
            p[_lib.POL_P_WEIGHTS + _lib.POL_TERMS.index(k)] = w
        self.params = p
        vp = C.c_void_p
        wc._call("tsidb_policy_config", p.ctypes.data_as(vp), _lib.POL_NPARAMS, self.action_scale.ctypes.data_as(vp),
                 self.default_joint_pos.ctypes.data_as(vp), self.term_body_mask)

        self.act_hist, self.last_action, self.prev_action = z(_lib.POL_HIST, N, NA), z(N, NA), z(N, NA)
        self.command, self.air_time, self.terms = z(N, 3), z(N, 2), z(N, _lib.POL_NT)
        self.ep_len, self.episode, self.timeout = z(N, dt=torch.int32), z(N, dt=torch.int32), z(N, dt=torch.int32)
        self.command[:] = torch.as_tensor(rng[:, 0], dtype=wc.dtype, device=wc.device)
        if delay is not None:
            if not isinstance(delay, torch.Tensor) or tuple(delay.shape) != (N,) or delay.dtype != torch.int32 \
                    or delay.device != wc.device or not delay.is_contiguous():
                raise _lib.TsidbError(f"PolicyEnv: delay must be a contiguous ({N},) int32 tensor on {wc.device}")
        self.delay = delay
        self._rows = z(N, self.NOBS + _lib.POL_NPRIV)
        self.obs, self.priv = self._rows[:, :self.NOBS], self._rows[:, self.NOBS:]
        self.reward, self.done = wc.reward, wc.done
        self._bufs = _lib.PolicyBufs(*(t.data_ptr() if t is not None else None for t in (
            self.act_hist, self.last_action, self.prev_action, self.command, self.air_time, self.ep_len, self.episode, self.delay,
            self.terms, self.timeout, self._rows)), self.NOBS + _lib.POL_NPRIV)
        if dr is not None:
            self.dr_params = dr
            wc._call("tsidb_policy_randomize", dr.ctypes.data_as(vp), _lib.POL_DR_NPARAMS)
            self._dr_push = bool(dr[_lib.POL_DR_PUSH_INTERVAL] >= 1 and dr[_lib.POL_DR_PUSH_DURATION] >= 1)
            self._dr_reset = bool(dr[_lib.POL_DR_RESET_JOINT_POS:_lib.POL_DR_RESET_LIFT + 1].any())
            if self._dr_push and wc.xfrc is None:
                wc.set_xfrc(z(N, wc.NB, 6))
        self.reset()   # (episode 1 starts)

    def written(self):
        """Every tensor a step() writes: what a caller that captures steps in a graph rewinds after its warm-up and keeps
        alive (WalkController._written lists the controller's)."""
        yield from self.wc._written()
        yield from (self.wc.ctrl, self.act_hist, self.last_action, self.prev_action, self.command, self.air_time, self.terms,
                    self.ep_len, self.episode, self.timeout, self._rows)
        if self.wc.xfrc is not None:
            yield self.wc.xfrc

    def _act(self, action):
        self.wc._call("tsidb_policy_act", C.byref(self._bufs), _ptr(action), self.wc._stream())

    def _reward(self):
        wc = self.wc
        wc._call("tsidb_policy_reward", C.byref(self._bufs), _ptr(wc.qpos), _ptr(wc.qvel), _ptr(wc.ncon), _ptr(wc.con_pairs),
                 _ptr(wc.info), _ptr(wc.reward), _ptr(wc.done), wc.NROW, wc._stream())

    def _obs(self):
        wc = self.wc
        wc._call("tsidb_policy_obs", C.byref(self._bufs), _ptr(wc.rows), wc.NROW, _ptr(wc.qpos), _ptr(wc.qvel), _ptr(wc.ncon),
                 _ptr(wc.con_pairs), wc._stream())

    def _perturb(self):
        self.wc._call("tsidb_policy_perturb", C.byref(self._bufs), self.wc._stream())

    def _reset_noise(self):
        wc = self.wc
        wc._call("tsidb_policy_reset_noise", C.byref(self._bufs), _ptr(wc.rows), wc.NROW, _ptr(wc.qpos), _ptr(wc.qvel), wc._stream())

    def reset(self, env_ids=None):
        """Restart the envs env_ids (None = all) as a done flag would: standing state, zeroed action history and air times, ctrl
        at the default pose (position mode), episode + 1, a new command where a range is set.  reward and done are cleared.
        Returns obs."""
        wc = self.wc
        wc.reward.zero_()
        wc.done.zero_()
        if env_ids is None:
            wc.done.fill_(1)
        else:
            ids = torch.as_tensor(env_ids, device=wc.device).long().reshape(-1)
            wc.done[ids] = 1
        wc.reset_done()
        if self._dr_reset:
            self._reset_noise()
        self._obs()
        wc.done.zero_()
        self.timeout.zero_()
        return self.obs

    def step(self, action):
        """One policy step for every env; action [N, NA] (self.dtype, on self.device, contiguous) in the actuator order.
        Returns (obs, reward, done, info): views updated in place; info = dict(timeout [N] int32: the episode ended by its
        length alone, terms [N, 12]: the unweighted reward terms, episode_length [N] int32: policy steps into the running
        episode, 0 for an env this step restarted).  obs is the FIRST observation of the new episode for a done env; reward,
        done and terms belong to the step that ended the old one.  With pushes on, info["push"] [N, 3] is the torso force the
        step applied (0 for an env it restarted: the reset clears the wrenches)."""
        wc = self.wc
        if action is None:
            raise _lib.TsidbError("PolicyEnv.step: action is None")
        wc._buffer("PolicyEnv.step", "action", (self.num_envs, self.NA), action)
        self._act(action)
        if self._dr_push:
            self._perturb()
        wc.sim_steps(self.decimation)
        self._reward()
        wc.reset_done()
        if self._dr_reset:
            self._reset_noise()
        self._obs()
        info = dict(timeout=self.timeout, terms=self.terms, episode_length=self.ep_len)
        if self._dr_push:
            info["push"] = wc.xfrc[:, 0, :3]
        return self.obs, self.reward, self.done, info
