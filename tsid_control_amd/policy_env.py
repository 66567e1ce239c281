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
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib
from .walk_controller import WalkController, _ptr


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
    sigma, h_target (None = the standing height), t_air, deadband, seed: the reward's constants.

    Tensors, all used in place: obs [N, NOBS], priv [N, 4] (base linear velocity in the body frame, base height), reward [N],
    done [N] (views of wc.rows), command [N, 3], delay [N], terms [N, 12], timeout [N], ep_len [N], episode [N], last_action,
    prev_action [N, NA], air_time [N, 2], act_hist [8, N, NA]; wc is the WalkController underneath."""

    def __init__(self, conf=None, num_envs=None, device=None, decimation=10, mode="position", action_scale=0.25,
                 default_joint_pos=None, action_clip=100.0, delay=None, filter_alpha=1.0, command_range=((0.0, 0.0),) * 3,
                 max_episode_steps=0, reward_weights=None, term_bodies=None, sigma=0.25, h_target=None, t_air=0.25, deadband=0.1,
                 seed=0):
        from .conf import RobotConfig
        conf = copy.copy(conf) if conf is not None else RobotConfig()
        conf.reference_quirks = False
        conf.sim_enabled = True
        if mode not in ("position", "motor"):
            raise _lib.TsidbError(f"PolicyEnv: mode must be 'position' or 'motor', got {mode!r}")
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
        self.reset()   # (episode 1 starts)

    def written(self):
        """Every tensor a step() writes: what a caller that captures steps in a graph rewinds after its warm-up and keeps
        alive (WalkController._written lists the controller's)."""
        yield from self.wc._written()
        yield from (self.wc.ctrl, self.act_hist, self.last_action, self.prev_action, self.command, self.air_time, self.terms,
                    self.ep_len, self.episode, self.timeout, self._rows)

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
        self._obs()
        wc.done.zero_()
        self.timeout.zero_()
        return self.obs

    def step(self, action):
        """One policy step for every env; action [N, NA] (self.dtype, on self.device, contiguous) in the actuator order.
        Returns (obs, reward, done, info): views updated in place; info = dict(timeout [N] int32: the episode ended by its
        length alone, terms [N, 12]: the unweighted reward terms, episode_length [N] int32: policy steps into the running
        episode, 0 for an env this step restarted).  obs is the FIRST observation of the new episode for a done env; reward,
        done and terms belong to the step that ended the old one."""
        wc = self.wc
        if action is None:
            raise _lib.TsidbError("PolicyEnv.step: action is None")
        wc._buffer("PolicyEnv.step", "action", (self.num_envs, self.NA), action)
        self._act(action)
        wc.sim_steps(self.decimation)
        self._reward()
        wc.reset_done()
        self._obs()
        return self.obs, self.reward, self.done, dict(timeout=self.timeout, terms=self.terms, episode_length=self.ep_len)
