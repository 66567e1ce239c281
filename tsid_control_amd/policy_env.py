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

With a PolicyTerrain two more launches join them: after the reset and its noise the sim's per-env tables - mass scale, contact
friction, floor plane, stepped terrain (WalkController.set_env_params) - are redrawn on the device for the envs just restarted
(tsidb_policy_terrain_reset), and after the observation a height scan of that floor around the base is written
(tsidb_policy_height_scan).  The same hash draws them, on streams of their own.

With tsid = "stand" or "walk" the batched TSID controller is in the loop: the sim stage of a step is `decimation` closed-loop env
steps (tick on the sim state, then sim; in "walk" each behind the walking reference update on a device clock) and two more
launches join the step - after the reward the teacher terms, TSID's failed QPs and its command as an action
(tsidb_policy_teacher), after the observation the controller's references in the base frame (tsidb_policy_teacher_obs).
mode = "residual" adds the policy's torque to TSID's tau; "position" / "motor" leave the sim to the policy and TSID beside it.

In those two modes the teacher can be learned from: rollout() into a RolloutStorage(teacher=True) records TSID's action as the
label of every stored row and, with teacher_beta, executes it in place of the policy's for that share of the episodes (DAgger's
mixing; one more launch per step, tsidb_policy_teacher_mix), and PolicyLearner(imitation_coef=...) has the term for the labels.

With episode_stats = True or a PolicyCurriculum two more launches join the step: right before the reset the running sums of the
episode, the record of every episode that ends and - with the curriculum - the terrain level of the env's next episode
(tsidb_policy_episode_end), behind the reset, its noise and the terrain's redraw the first position of the episodes that start
(tsidb_policy_episode_begin).  episode_stats() turns the per-env sums into what a training loop logs, without a host read.

With a PolicyObsHistory one more launch closes the step (tsidb_policy_obs_history; csrc/tsidb_history.hpp): the observation it
just wrote becomes the newest of the last `frames` frames in obs_history, the stacked row a feed-forward actor reads as a memory.
"""
import copy
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .walk_controller import WalkController, _ptr


def _of(cls, r, what, fields):
    """r as a cls: one, or a dict of its fields (`what`: the PolicyEnv argument, for the messages)"""
    if isinstance(r, cls):
        return r
    if not isinstance(r, dict):
        raise _lib.TsidbError(f"PolicyEnv: {what} must be a {cls.__name__} or a dict, got {type(r).__name__}")
    unknown = sorted(set(r) - set(fields))
    if unknown:
        raise _lib.TsidbError(f"PolicyEnv: unknown {what} fields {unknown} (known: {fields})")
    return cls(**r)


def _weight_vector(weights, terms, what):
    """{term: weight} as the weights in the order of `terms`, 0 for a term left out"""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(terms))
    if unknown:
        raise _lib.TsidbError(f"PolicyEnv: unknown {what} terms {unknown} (known: {terms})")
    return [weights.get(k, 0.0) for k in terms]


def _whole_below(who, name, v, bits):
    """v as an int if it is a finite whole number in [0, 2^bits) - what the library asks of seeds, offsets, intervals and counts"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v != math.floor(v) or not 0 <= v < 2 ** bits:
        raise _lib.TsidbError(f"{who}: {name} must be a whole number in [0, 2^{bits}), got {v!r}")
    return int(v)


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
        return _of(cls, r, "randomization", _lib.POL_DR_FIELDS)

    def params(self, default_seed=0):
        """the float64 vector tsidb_policy_randomize takes, checked as the library checks it"""
        p = np.zeros(_lib.POL_DR_NPARAMS)
        for k in _lib.POL_DR_FIELDS:
            v = default_seed if k == "seed" and self.seed is None else getattr(self, k)
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
            _whole_below("PolicyRandomization", k, p[getattr(_lib, "POL_DR_" + k.upper())], 32 if k == "seed" else 31)
        if p[_lib.POL_DR_PUSH_DURATION] > p[_lib.POL_DR_PUSH_INTERVAL]:
            raise bad("push_duration > push_interval")
        if p[_lib.POL_DR_PUSH_FORCE_LO] > p[_lib.POL_DR_PUSH_FORCE_HI]:
            raise bad("push_force_lo > push_force_hi")
        if p[_lib.POL_DR_COMMAND_ZERO_PROB] > 1:
            raise bad("command_zero_prob must be in [0, 1]")
        return p


@dataclasses.dataclass
class PolicyTerrain:
    """Per-episode dynamics and terrain of a PolicyEnv and its height scan (include/tsidb.h TSIDB_POL_TER_*).  seed: of these
    draws (None = the env's seed; below 2^32).  env_offset: added to the env index in every draw (None = the randomization's,
    else 0).  Ranges are (lo, hi), drawn uniformly at every restart, lo == hi = that value: mass (scale of every sim body's mass
    and inertia, > 0), friction (floor contacts, > 0), step_height [m] (of the raised strips, scaled by (level + 1) / num_levels
    with level = PolicyEnv.terrain_level of the env), step_length [m] (width of a strip, > 0).  tilt_deg: the floor is a plane
    through the point under the restarted robot, tilted by at most this much (< 45) about a random azimuth.  step_prob: each
    of the 16 strips of the stepped floor, which repeat along a random direction, is raised with this probability; the strip
    under the restarted robot and flat_cells (0 .. 7) strips on each side of it stay level.  scan_x, scan_y: (first, last,
    points) of the height scan's grid along the base's heading and to its left [m], None = no scan (both or neither; at most 256
    points); scan_clip: (lo, hi) the base's height above the surface is clipped to; scan_noise [m]: uniform in +-scan_noise, added
    after the clip."""
    seed: int = None
    env_offset: int = None
    mass: object = (1.0, 1.0)
    friction: object = (1.0, 1.0)
    tilt_deg: float = 0.0
    step_height: object = (0.0, 0.0)
    step_length: object = (0.08, 0.08)
    step_prob: float = 0.5
    flat_cells: int = 1
    num_levels: int = 1
    scan_x: object = None
    scan_y: object = None
    scan_clip: object = (-1.0, 1.0)
    scan_noise: float = 0.0

    @classmethod
    def of(cls, t):
        """t as a PolicyTerrain: one, or a dict of its fields"""
        return _of(cls, t, "terrain", _lib.POL_TER_FIELDS)

    def params(self, default_seed=0, default_env_offset=0):
        """the float64 vector tsidb_policy_terrain_config takes, checked as the library checks it"""
        bad = lambda msg: _lib.TsidbError("PolicyTerrain: " + msg)

        def numbers(k, count):
            v = getattr(self, k)
            try:
                a = np.asarray(v, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError) as err:
                raise bad(f"{k} = {v!r} is not {count} numbers") from err
            if a.shape != (count,):
                raise bad(f"{k} = {v!r} is not {count} numbers")
            return a

        p = np.zeros(_lib.POL_TER_NPARAMS)
        seed = default_seed if self.seed is None else self.seed
        offset = default_env_offset if self.env_offset is None else self.env_offset
        scalars = dict(seed=seed, env_offset=offset, tilt_deg=self.tilt_deg, step_prob=self.step_prob, flat_cells=self.flat_cells,
                       num_levels=self.num_levels, scan_noise=self.scan_noise)
        for k, v in scalars.items():
            try:
                scalars[k] = float(v)
            except (TypeError, ValueError) as err:
                raise bad(f"{k} = {v!r} is not a number") from err
        p[_lib.POL_TER_SEED], p[_lib.POL_TER_ENV_OFFSET] = scalars["seed"], scalars["env_offset"]
        p[_lib.POL_TER_TILT_MAX] = math.radians(scalars["tilt_deg"])
        p[_lib.POL_TER_STEP_PROB], p[_lib.POL_TER_SCAN_NOISE] = scalars["step_prob"], scalars["scan_noise"]
        p[_lib.POL_TER_FLAT_CELLS], p[_lib.POL_TER_NUM_LEVELS] = scalars["flat_cells"], scalars["num_levels"]
        for k, i in (("mass", _lib.POL_TER_MASS_LO), ("friction", _lib.POL_TER_FRICTION_LO), ("step_height", _lib.POL_TER_STEP_HEIGHT_LO),
                     ("step_length", _lib.POL_TER_STEP_LENGTH_LO), ("scan_clip", _lib.POL_TER_SCAN_CLIP_LO)):
            p[i:i + 2] = numbers(k, 2)
        for k, i, j in (("scan_x", _lib.POL_TER_SCAN_X0, _lib.POL_TER_SCAN_NX), ("scan_y", _lib.POL_TER_SCAN_Y0, _lib.POL_TER_SCAN_NY)):
            if getattr(self, k) is not None:
                p[i], p[i + 1], p[j] = numbers(k, 3)
        if not np.isfinite(p).all():
            raise bad("non-finite value")
        for k in ("seed", "env_offset", "flat_cells", "num_levels", "scan_nx", "scan_ny"):
            _whole_below("PolicyTerrain", k, p[getattr(_lib, "POL_TER_" + k.upper())], 32 if k == "seed" else 31)
        for k, i in (("mass", _lib.POL_TER_MASS_LO), ("friction", _lib.POL_TER_FRICTION_LO), ("step_height", _lib.POL_TER_STEP_HEIGHT_LO),
                     ("step_length", _lib.POL_TER_STEP_LENGTH_LO), ("scan_clip", _lib.POL_TER_SCAN_CLIP_LO)):
            if p[i] > p[i + 1]:
                raise bad(f"{k}: lo > hi")
        for k, i in (("mass", _lib.POL_TER_MASS_LO), ("friction", _lib.POL_TER_FRICTION_LO), ("step_length", _lib.POL_TER_STEP_LENGTH_LO)):
            if not p[i] > 0:
                raise bad(f"{k} must be positive")
        if not 0 <= p[_lib.POL_TER_TILT_MAX] < math.pi / 4:
            raise bad("tilt_deg must be in [0, 45)")
        if p[_lib.POL_TER_STEP_HEIGHT_LO] < 0:
            raise bad("step_height must be >= 0")
        if not 0 <= p[_lib.POL_TER_STEP_PROB] <= 1:
            raise bad("step_prob must be in [0, 1]")
        if p[_lib.POL_TER_FLAT_CELLS] > 7:
            raise bad("flat_cells must be 0 .. 7")
        if p[_lib.POL_TER_NUM_LEVELS] < 1:
            raise bad("num_levels must be a whole number >= 1 (below 2^31)")
        nx, ny = p[_lib.POL_TER_SCAN_NX], p[_lib.POL_TER_SCAN_NY]
        if (nx == 0) != (ny == 0):
            raise bad("scan_x and scan_y must both be given, with at least one point each, or neither")
        if nx * ny > _lib.POL_MAXSCAN:
            raise bad(f"the scan has {int(nx * ny)} points, at most {_lib.POL_MAXSCAN}")
        if p[_lib.POL_TER_SCAN_NOISE] < 0:
            raise bad("scan_noise must be >= 0")
        return p


@dataclasses.dataclass
class PolicyCurriculum:
    """The terrain curriculum of a PolicyEnv (include/tsidb.h tsidb_policy_episode_end, TSIDB_POL_EPP_*): legged_gym's rule on
    PolicyEnv.terrain_level, applied on the device to every env whose episode ends.  With d the distance of the base from where
    the episode started: d > up_distance [m] moves the env one level up; otherwise d < down_fraction x the distance its command
    asked for over a whole episode (|command_xy| max_episode_steps decimation dt) moves it one level down.  A level below 0
    stays 0; an env that graduates from the top level gets a uniformly drawn level (random_top) or stays at the top."""
    up_distance: float
    down_fraction: float = 0.5
    random_top: bool = True

    @classmethod
    def of(cls, c):
        """c as a PolicyCurriculum: one, or a dict of its fields"""
        return _of(cls, c, "curriculum", _lib.POL_CURRICULUM_FIELDS)

    def params(self):
        """the float64 vector tsidb_policy_episode_config takes (the curriculum on), checked as the library checks it"""
        bad = lambda msg: _lib.TsidbError("PolicyCurriculum: " + msg)
        if not isinstance(self.random_top, (bool, np.bool_)) and self.random_top not in (0, 1):
            raise bad(f"random_top must be True or False, got {self.random_top!r}")
        p = np.zeros(_lib.POL_EPP_NPARAMS)
        try:
            p[_lib.POL_EPP_UP_DISTANCE], p[_lib.POL_EPP_DOWN_FRACTION] = float(self.up_distance), float(self.down_fraction)
        except (TypeError, ValueError) as err:
            raise bad(f"up_distance = {self.up_distance!r}, down_fraction = {self.down_fraction!r}: not numbers") from err
        p[_lib.POL_EPP_CURRICULUM], p[_lib.POL_EPP_RANDOM_TOP] = 1.0, float(bool(self.random_top))
        if not np.isfinite(p).all():
            raise bad("non-finite value")
        if not p[_lib.POL_EPP_UP_DISTANCE] > 0:
            raise bad("up_distance must be positive")
        if p[_lib.POL_EPP_DOWN_FRACTION] < 0:
            raise bad("down_fraction must be >= 0")
        return p


@dataclasses.dataclass
class PolicyObsHistory:
    """The observation history of a PolicyEnv (include/tsidb.h tsidb_policy_obs_history): PolicyEnv.obs_history [N, frames * K],
    the last `frames` observations of every env, frame-major, oldest first.  frames: 1 .. 32.  sources: 1 .. 4 entries, each the
    name of one of the env's tensors - "obs", "priv", "command", "height_scan", "teacher_obs" - or (name, lo, hi), its columns
    lo .. hi - 1; a frame is their concatenation in the order given, K columns, and the same name may come twice with different
    ranges.  frames * K may be up to 4096; a PolicyActor's input row holds 512 columns."""
    frames: int
    sources: object = ("obs",)

    @classmethod
    def of(cls, h):
        """h as a PolicyObsHistory: one, or a dict of its fields"""
        return _of(cls, h, "obs_history", _lib.POL_OBSH_FIELDS)

    def resolve(self, columns):
        """[(name, lo, hi)] of the sources, checked as the library checks them; columns: {name: the columns of the env's tensor,
        or a str saying why the env has none}.  K is the sum of hi - lo."""
        bad = lambda msg: _lib.TsidbError("PolicyObsHistory: " + msg)
        f = self.frames
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or f != math.floor(f) \
                or not 1 <= f <= _lib.POL_OBSH_MAXFRAMES:
            raise bad(f"frames must be a whole number in 1 .. {_lib.POL_OBSH_MAXFRAMES}, got {f!r}")
        sources = (self.sources,) if isinstance(self.sources, str) else self.sources
        if not isinstance(sources, (list, tuple)) or not 1 <= len(sources) <= _lib.POL_OBSH_MAXSRC:
            raise bad(f"sources must be a list of 1 .. {_lib.POL_OBSH_MAXSRC} entries, got {self.sources!r}")
        out = []
        for s in sources:
            name, rng = (s, None) if isinstance(s, str) else (s[0], tuple(s[1:])) if isinstance(s, (list, tuple)) and len(s) == 3 else (None, None)
            if name not in _lib.POL_OBSH_SOURCES:
                raise bad(f"unknown source {s!r} (a source is a name of {_lib.POL_OBSH_SOURCES} or (name, lo, hi))")
            n = columns[name]
            if isinstance(n, str):
                raise bad(f"the env has no {name} ({n})")
            lo, hi = (0, n) if rng is None else rng
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (lo, hi)) or not 0 <= lo < hi <= n:
                raise bad(f"column range ({lo!r}, {hi!r}) of {name} must be whole numbers with 0 <= lo < hi <= {n}")
            out.append((name, int(lo), int(hi)))
        total = int(f) * sum(hi - lo for _, lo, hi in out)
        if total > _lib.POL_OBSH_MAXCOLS:
            raise bad(f"frames * K = {total} columns, at most {_lib.POL_OBSH_MAXCOLS}")
        return out


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
    prev_action [N, NA], air_time [N, 2], act_hist [8, N, NA]; wc is the WalkController underneath.

    tsid: None (no tick: the environment above), "stand" or "walk" - TSID in the loop; conf must then have closed_loop = True
    (walk_planner.op3_closed_loop_walking_conf for walking).  "stand": one wc.step(decimation) per policy step.  "walk": per sim
    step the walking reference update at the device clock self.clock (float64 [1]), one closed-loop env step, clock += dt;
    self.sched is the WalkSchedule.on_device(wc, **walk) the env builds - walk: its keyword arguments (default foot_press = 0)
    plus touchdown_feedback (fraction of the swing, default 0.6; None = off) and posture_bias ([NA] added to the posture
    reference, default walk_planner.op3_walking_posture() for the 20-actuator robot); the envs a step or reset() restarts are
    replanned on a new path with their clocks at self.clock.  mode "residual" (only with tsid): ctrl = default_joint_pos
    (default 0) + action_scale * action is a torque [N m] added to TSID's tau.  teacher_weights: {term: weight} over
    _lib.POL_TEACH_TERMS added to the reward, sigma_com / sigma_foot [m] the widths of the two tracking terms (a reset leaves
    the foot references at the identity placement and only a walking schedule writes them: track_feet and the foot errors of
    teacher_obs mean something with tsid = "walk").  Reset noise
    that moves the base (reset_xy, reset_yaw, reset_lift) is rejected with tsid: the plan and the contact references start
    where the reset put the robot.  More tensors: teacher_terms [N, 4], teacher_action [N, NA], teacher_obs [N, 14 + NA]
    (include/tsidb.h tsidb_policy_teacher / _teacher_obs), all three in step()'s info.

    terrain: a PolicyTerrain or a dict of its fields (None = none: the launches and every result are those of an env built
    without the argument).  The env registers nominal tables once (wc.set_env_params(mass_scale=1, terrain="flat")) and the
    kernels rewrite wc.env_params [N, 8] and wc.terrain [N, 20] in place, for the envs a step or reset() restarts.  terrain_level
    [N] int32, zero at first, is the caller's to write: the level of the env's NEXT episodes (the hook of a terrain curriculum;
    curriculum= below writes it on the device, otherwise no promotion rule runs).  height_scan [N, nx * ny]: point ix * ny + iy.  All three are in step()'s info (env_params
    under that name).  Accepted with tsid = "stand" / "walk", but the controller is NOT told about the floor: its references,
    contact frames and plan assume the level floor z = 0, so a tilt or steps are a disturbance TSID has to absorb.

    episode_stats = True: two more launches per step keep what a training loop logs (include/tsidb.h tsidb_policy_episode_end
    before the reset, _begin behind it): episode_last [N, NREC] float64, the record of each env's most recently finished
    episode (columns _lib.POL_EP_*: count, timeout, length, return, displacement, level, the 12 term sums, the 4 teacher term
    sums), and episode_sum [N, NREC], the per-env sums of the records since episode_stats() last cleared them; both in step()'s
    info.  episode_run [N, NREC] and episode_start_xy [N, 2] are the running episode's state.  reset() starts the episodes it
    forces and records nothing for the ones it abandons.  curriculum: a PolicyCurriculum or a dict of its fields (None =
    none); implies episode_stats, needs terrain= and max_episode_steps > 0: the same launch then writes terrain_level, the level
    of each done env's next episode, before the terrain's redraw reads it.

    obs_history: a PolicyObsHistory or a dict of its fields (None = none: the launches and every result are those of an env
    built without the argument).  One more launch closes step() and reset() (include/tsidb.h tsidb_policy_obs_history) and keeps
    obs_history [N, frames * K] in the env's dtype: the last `frames` selections of the named tensors, frame-major, oldest
    first - frame h is columns h K .. (h + 1) K, the newest frame is the current selection.  Frames are copies of what the
    observation kernels left, noise included.  An env a step or reset() restarts holds `frames` copies of its first
    observation; reset() leaves the history of the envs it does not restart as it is (it is no new time step).  The tensor is
    in step()'s info, and "obs_history" is an input block of a PolicyActor - so rollout() runs with a history as it is.
    obs_history_spec is the PolicyObsHistory, obs_history_sources its sources resolved to [(name, lo, hi)]."""

    # the randomisation's launches a step makes; class-level so that an instance built without __init__ steps unrandomised
    randomization = None
    _dr_push = _dr_reset = False
    # per-episode terrain and dynamics, the height scan: class-level for the same reason
    terrain = terrain_level = height_scan = None
    # TSID in the loop: None = no tick; sched = the walking schedule of tsid = "walk", clock its device time
    tsid = sched = clock = None
    # the [1] float32 device tensor behind rollout(teacher_beta = a float), made at the first such call
    _teacher_beta = None
    # episode statistics and the terrain curriculum: _episode = the tsidb_policy_episode block, None = the slice is off
    curriculum = _episode = episode_run = episode_start_xy = episode_last = episode_sum = None
    # the observation history: obs_history = the [N, frames * K] tensor, _obs_history = the tsidb_policy_obs_history block;
    # None = off
    obs_history = _obs_history = None

    def __init__(self, conf=None, num_envs=None, device=None, decimation=10, mode="position", action_scale=0.25,
                 default_joint_pos=None, action_clip=100.0, delay=None, filter_alpha=1.0, command_range=((0.0, 0.0),) * 3,
                 max_episode_steps=0, reward_weights=None, term_bodies=None, sigma=0.25, h_target=None, t_air=0.25, deadband=0.1,
                 seed=0, randomization=None, tsid=None, walk=None, teacher_weights=None, sigma_com=0.05, sigma_foot=0.05, terrain=None,
                 episode_stats=False, curriculum=None, obs_history=None):
        from .conf import RobotConfig
        conf = copy.copy(conf) if conf is not None else RobotConfig()
        conf.reference_quirks = False
        conf.sim_enabled = True
        if tsid not in (None, "stand", "walk"):
            raise _lib.TsidbError(f"PolicyEnv: tsid must be None, 'stand' or 'walk', got {tsid!r}")
        if mode not in ("position", "motor") and not (mode == "residual" and tsid is not None):
            raise _lib.TsidbError(f"PolicyEnv: mode must be 'position' or 'motor', or 'residual' with tsid = 'stand' / 'walk' "
                                  f"(a residual needs TSID's tau to add to), got {mode!r}")
        # the four parameter vectors: checked before anything is built
        self.params = base = self._base_params(int(decimation), action_clip, filter_alpha, sigma, t_air, deadband, max_episode_steps, seed,
                                               command_range, reward_weights)
        dr = ter = teach = epp = None
        if randomization is not None:
            self.randomization = PolicyRandomization.of(randomization)
            dr = self.randomization.params(seed)
        if terrain is not None:
            self.terrain = PolicyTerrain.of(terrain)
            ter = self.terrain.params(seed, 0 if dr is None else int(dr[_lib.POL_DR_ENV_OFFSET]))
        if curriculum is not None:
            self.curriculum = PolicyCurriculum.of(curriculum)
            epp = self.curriculum.params()
            if ter is None or not base[_lib.POL_P_MAX_EPISODE_STEPS] > 0:
                raise _lib.TsidbError("PolicyEnv: a curriculum needs terrain= (the levels are the terrain's) and max_episode_steps > 0 "
                                      "(the distance a command asks for is over a whole episode)")
        elif episode_stats:
            epp = np.zeros(_lib.POL_EPP_NPARAMS)
        if tsid is None:
            if walk is not None or teacher_weights:
                raise _lib.TsidbError("PolicyEnv: walk and teacher_weights need tsid = 'stand' or 'walk'")
        else:
            if not getattr(conf, "closed_loop", False):
                raise _lib.TsidbError("PolicyEnv: tsid needs a closed-loop conf (conf.closed_loop = True; for walking "
                                      "walk_planner.op3_closed_loop_walking_conf): the tick must read the sim state the policy moves")
            if walk is not None and tsid != "walk":
                raise _lib.TsidbError("PolicyEnv: walk is the schedule's arguments of tsid = 'walk'")
            teach = self._teacher_params(teacher_weights, sigma_com, sigma_foot)
            moved = [k for k in ("reset_xy", "reset_yaw", "reset_lift") if dr is not None and dr[getattr(_lib, "POL_DR_" + k.upper())] != 0]
            if moved:
                raise _lib.TsidbError(f"PolicyEnv: {', '.join(moved)} cannot be used with tsid: the walking plan and the contact "
                                      "references start from the base pose the reset captured (joint and velocity noise are fine: "
                                      "the closed-loop tick reads the sim state)")
        if obs_history is not None:
            from .model import ModelBlob
            self.obs_history_spec = PolicyObsHistory.of(obs_history)
            na = int(ModelBlob(getattr(conf, "model_blob", None))["model_dims"][3])   # (the controller is not built yet)
            scan = 0 if ter is None else int(ter[_lib.POL_TER_SCAN_NX] * ter[_lib.POL_TER_SCAN_NY])
            self.obs_history_sources = self.obs_history_spec.resolve(dict(
                obs=_lib.pol_nobs(na), priv=_lib.POL_NPRIV, command=3, height_scan=scan or "it needs terrain= with scan_x and scan_y",
                teacher_obs=_lib.pol_teach_nobs(na) if tsid is not None else "it needs tsid = 'stand' or 'walk'"))
        # the controller
        self.wc = wc = WalkController(conf, num_envs=num_envs, device=device)
        self.num_envs, self.device, self.dtype, self.NA = wc.num_envs, wc.device, wc.dtype, wc.NA
        N, NA = wc.num_envs, wc.NA
        self.NOBS = _lib.pol_nobs(NA)
        self.decimation, self.mode, self.tsid = int(decimation), mode, tsid
        base[_lib.POL_P_H_TARGET] = float(wc.qpos[0, 2]) if h_target is None else h_target
        if default_joint_pos is None:
            default_joint_pos = wc.ctrl_from_q(wc.q0)[0].double().cpu().numpy() if mode == "position" else 0.0
        self.action_scale = np.broadcast_to(np.asarray(action_scale, dtype=np.float64), (NA,)).copy()
        self.default_joint_pos = np.broadcast_to(np.asarray(default_joint_pos, dtype=np.float64), (NA,)).copy()
        self.term_body_mask = 1 if term_bodies is None else sum(1 << int(b) for b in set(term_bodies))
        if delay is not None and (not isinstance(delay, torch.Tensor) or tuple(delay.shape) != (N,) or delay.dtype != torch.int32
                                  or delay.device != wc.device or not delay.is_contiguous()):
            raise _lib.TsidbError(f"PolicyEnv: delay must be a contiguous ({N},) int32 tensor on {wc.device}")
        self.delay = delay
        # the tensors
        z = lambda *s, dt=wc.dtype: torch.zeros(*s, dtype=dt, device=wc.device)
        self.act_hist, self.last_action, self.prev_action = z(_lib.POL_HIST, N, NA), z(N, NA), z(N, NA)
        self.command, self.air_time, self.terms = z(N, 3), z(N, 2), z(N, _lib.POL_NT)
        self.ep_len, self.episode, self.timeout = z(N, dt=torch.int32), z(N, dt=torch.int32), z(N, dt=torch.int32)
        self.command[:] = torch.as_tensor(base[_lib.POL_P_CMD_LO:_lib.POL_P_CMD_LO + 3], dtype=wc.dtype, device=wc.device)
        self._rows = z(N, self.NOBS + _lib.POL_NPRIV)
        self.obs, self.priv = self._rows[:, :self.NOBS], self._rows[:, self.NOBS:]
        self.reward, self.done = wc.reward, wc.done
        self._bufs = _lib.PolicyBufs(*(t.data_ptr() if t is not None else None for t in (
            self.act_hist, self.last_action, self.prev_action, self.command, self.air_time, self.ep_len, self.episode, self.delay,
            self.terms, self.timeout, self._rows)), self.NOBS + _lib.POL_NPRIV)
        if ter is not None:
            self.terrain_level, self.height_scan = z(N, dt=torch.int32), z(N, int(ter[_lib.POL_TER_SCAN_NX] * ter[_lib.POL_TER_SCAN_NY]))
        if tsid is not None:
            self.teacher_terms, self.teacher_action, self.teacher_obs = z(N, _lib.POL_TEACH_NT), z(N, NA), z(N, _lib.pol_teach_nobs(NA))
        # the library's configuration, group by group
        vec = lambda p: (p.ctypes.data_as(C.c_void_p), len(p))
        wc.set_ctrl(z(N, NA), mode)
        if base[_lib.POL_P_WEIGHTS + _lib.POL_TERMS.index("torques")] != 0.0:     # the readout kernels cost 3-4 %: only when the term is used
            wc.enable_sim_readouts()
        wc._call("tsidb_policy_config", *vec(base), self.action_scale.ctypes.data_as(C.c_void_p),
                 self.default_joint_pos.ctypes.data_as(C.c_void_p), self.term_body_mask)
        if dr is not None:
            self.dr_params = dr
            wc._call("tsidb_policy_randomize", *vec(dr))
            self._dr_push = bool(dr[_lib.POL_DR_PUSH_INTERVAL] >= 1 and dr[_lib.POL_DR_PUSH_DURATION] >= 1)
            self._dr_reset = bool(dr[_lib.POL_DR_RESET_JOINT_POS:_lib.POL_DR_RESET_LIFT + 1].any())
            if self._dr_push and wc.xfrc is None:
                wc.set_xfrc(z(N, wc.NB, 6))
        if ter is not None:
            self.ter_params = ter
            wc.set_env_params(mass_scale=1.0, terrain="flat")      # nominal rows; the kernels rewrite the two tensors in place
            wc._call("tsidb_policy_terrain_config", *vec(ter))
        if tsid is not None:
            self.teach_params = teach
            wc._call("tsidb_policy_teacher_config", *vec(teach))
            if tsid == "walk":
                self._build_schedule(dict(walk or {}))
        if epp is not None:
            self.ep_params = epp
            d = lambda *s: torch.zeros(*s, dtype=torch.float64, device=wc.device)   # float64 whatever the path's dtype
            self.episode_run, self.episode_start_xy = d(N, _lib.POL_EP_NREC), d(N, 2)
            self.episode_last, self.episode_sum = d(N, _lib.POL_EP_NREC), d(N, _lib.POL_EP_NREC)
            self._episode = _lib.PolicyEpisode(*(t.data_ptr() if t is not None else None for t in (
                self.episode_run, self.episode_start_xy, self.episode_last, self.episode_sum, self.terrain_level,
                self.teacher_terms if tsid is not None else None)))
            wc._call("tsidb_policy_episode_config", *vec(epp))
        if obs_history is not None:
            self._build_obs_history()
        self.reset()   # (episode 1 starts: every env's history is filled with its first observation)

    @staticmethod
    def _base_params(decimation, action_clip, filter_alpha, sigma, t_air, deadband, max_episode_steps, seed, command_range, reward_weights):
        """the float64 vector tsidb_policy_config takes, which checks its values; h_target is left to __init__: its default needs the
        controller"""
        p = np.zeros(_lib.POL_NPARAMS)
        p[_lib.POL_P_CLIP], p[_lib.POL_P_ALPHA], p[_lib.POL_P_SIGMA] = action_clip, filter_alpha, sigma
        p[_lib.POL_P_T_AIR], p[_lib.POL_P_DEADBAND] = t_air, deadband
        p[_lib.POL_P_MAX_EPISODE_STEPS], p[_lib.POL_P_DECIMATION], p[_lib.POL_P_SEED] = max_episode_steps, decimation, seed
        rng = np.asarray(command_range, dtype=np.float64).reshape(3, 2)
        p[_lib.POL_P_CMD_LO:_lib.POL_P_CMD_LO + 3], p[_lib.POL_P_CMD_HI:_lib.POL_P_CMD_HI + 3] = rng[:, 0], rng[:, 1]
        p[_lib.POL_P_WEIGHTS:] = _weight_vector(reward_weights, _lib.POL_TERMS, "reward")
        return p

    @staticmethod
    def _teacher_params(teacher_weights, sigma_com, sigma_foot):
        """the float64 vector tsidb_policy_teacher_config takes, checked as the library checks it"""
        p = np.zeros(_lib.POL_TEACH_NPARAMS)
        p[_lib.POL_TEACH_SIGMA_COM], p[_lib.POL_TEACH_SIGMA_FOOT] = sigma_com, sigma_foot
        p[_lib.POL_TEACH_WEIGHTS:] = _weight_vector(teacher_weights, _lib.POL_TEACH_TERMS, "teacher")
        if not np.isfinite(p).all():
            raise _lib.TsidbError("PolicyEnv: non-finite teacher weight or sigma")
        if not (p[_lib.POL_TEACH_SIGMA_COM] > 0 and p[_lib.POL_TEACH_SIGMA_FOOT] > 0):
            raise _lib.TsidbError(f"PolicyEnv: sigma_com and sigma_foot must be positive, got {sigma_com}, {sigma_foot}")
        return p

    def _build_schedule(self, walk):
        """tsid = "walk": the device clock and the schedule"""
        from .walk_planner import WalkSchedule, op3_walking_posture
        wc = self.wc
        fraction = walk.pop("touchdown_feedback", 0.6)
        bias = walk.pop("posture_bias", op3_walking_posture() if wc.NA == 20 else None)
        walk.setdefault("foot_press", 0.0)
        if bias is not None:
            wc.set_posture_bias(bias)
        self.clock = torch.zeros(1, dtype=torch.float64, device=wc.device)   # float64 whatever the path's dtype
        self.sched = WalkSchedule.on_device(wc, plan=False, **walk)
        if fraction is not None:
            self.sched.enable_touchdown_feedback(fraction)     # (reset() plans: every env is restarted before the first step)

    def _build_obs_history(self):
        """the history tensor and the block the launch takes: each source a column range of one of the env's tensors"""
        item = self._rows.element_size()
        frame = {"obs": (self._rows, 0), "priv": (self._rows, self.NOBS), "command": (self.command, 0),
                 "height_scan": (self.height_scan, 0), "teacher_obs": (getattr(self, "teacher_obs", None), 0)}
        h = _lib.PolicyObsHistory()
        h.frames, h.n_src = int(self.obs_history_spec.frames), len(self.obs_history_sources)
        for i, (name, lo, hi) in enumerate(self.obs_history_sources):
            t, first = frame[name]
            h.src[i], h.src_ld[i], h.src_cols[i] = t.data_ptr() + (first + lo) * item, int(t.stride(0)), hi - lo
        K = sum(hi - lo for _, lo, hi in self.obs_history_sources)
        self.obs_history = torch.zeros(self.num_envs, h.frames * K, dtype=self.wc.dtype, device=self.wc.device)
        h.history = self.obs_history.data_ptr()
        self._obs_history = h

    def written(self):
        """Every tensor a step() writes: what a caller that captures steps in a graph rewinds after its warm-up and keeps
        alive (WalkController._written lists the controller's)."""
        yield from self.wc._written()
        yield from (self.wc.ctrl, self.act_hist, self.last_action, self.prev_action, self.command, self.air_time, self.terms,
                    self.ep_len, self.episode, self.timeout, self._rows)
        if self.wc.xfrc is not None:
            yield self.wc.xfrc
        if self.terrain is not None:
            yield from (self.wc.env_params, self.wc.terrain, self.height_scan)
        if self.tsid is not None:
            yield from (self.teacher_terms, self.teacher_action, self.teacher_obs)
        if self.sched is not None:
            s = self.sched
            yield from (self.clock, s.td_latch, s.coef, s.rest, s.com, s.side, s.nsteps, s.steps, s.flags, s.episode, s.t_offset)
        if self._episode is not None:
            yield from (self.episode_run, self.episode_start_xy, self.episode_last, self.episode_sum)
            if self.curriculum is not None:
                yield self.terrain_level
        if self._obs_history is not None:
            yield self.obs_history

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

    def _terrain_reset(self):
        wc = self.wc
        wc._call("tsidb_policy_terrain_reset", C.byref(self._bufs), _ptr(wc.rows), wc.NROW, _ptr(wc.qpos), _ptr(self.terrain_level),
                 wc._stream())

    def _height_scan(self):
        wc = self.wc
        wc._call("tsidb_policy_height_scan", C.byref(self._bufs), _ptr(wc.qpos), _ptr(self.height_scan), self.height_scan.shape[1],
                 wc._stream())

    def _tsid_steps(self):
        """`decimation` closed-loop env steps: tick on the sim state, then sim - in "walk" each behind its reference update"""
        wc = self.wc
        if self.sched is None:
            wc.step(self.decimation)
            return
        dt = wc.conf.dt
        for _ in range(self.decimation):
            self.sched.apply(wc, 0.0, t_device=self.clock)
            wc.step(1)
            self.clock += dt

    def _replan(self):
        """the envs reset_done just restarted get a new path, and their plans start at the clock"""
        self.sched.plan(self.wc, done_only=True, new_paths=True, t_device=self.clock)

    def _teacher(self):
        wc = self.wc
        wc._call("tsidb_policy_teacher", C.byref(self._bufs), _ptr(wc.rows), wc.NROW, _ptr(wc.q), _ptr(wc.tau), _ptr(wc.status),
                 _ptr(wc.ncon), _ptr(wc.con_pairs), _ptr(self.teacher_terms), _ptr(self.teacher_action), wc._stream())

    def _teacher_obs(self):
        wc = self.wc
        wc._call("tsidb_policy_teacher_obs", C.byref(self._bufs), _ptr(wc.rows), wc.NROW, _ptr(wc.qpos), _ptr(wc.tau),
                 _ptr(self.teacher_obs), self.teacher_obs.shape[1], wc._stream())

    def _teacher_mix(self, actor, action, label, weight, executed, beta):
        """one tsidb_policy_teacher_mix launch: labels, weights and executed flags of this step into the three tensors, and the
        teacher's action over `action` (None: not touched) for the envs whose episode the draw gives to the teacher; beta: a [1]
        float32 device tensor or None (= 0); the seed and the env offset are the actor's, as for its action noise"""
        self.wc._call("tsidb_policy_teacher_mix", C.byref(self._bufs), _ptr(self.teacher_action), _ptr(action),
                      _ptr(label), _ptr(weight), _ptr(executed), _ptr(beta), C.c_uint64(actor.seed),
                      C.c_uint64(actor.env_offset), self.wc._stream())

    def _episode_end(self):
        wc = self.wc
        wc._call("tsidb_policy_episode_end", C.byref(self._bufs), C.byref(self._episode), _ptr(wc.qpos), _ptr(wc.reward), _ptr(wc.done),
                 wc.NROW, wc._stream())

    def _episode_begin(self):
        wc = self.wc
        wc._call("tsidb_policy_episode_begin", C.byref(self._bufs), C.byref(self._episode), _ptr(wc.rows), wc.NROW, _ptr(wc.qpos),
                 wc._stream())

    def _push_obs_history(self, push):
        wc = self.wc
        wc._call("tsidb_policy_obs_history", C.byref(self._obs_history), _ptr(wc.rows), wc.NROW, int(push), wc._stream())

    def episode_stats(self, clear=True):
        """What the episodes that finished since the last clear amount to, as 0-dim float64 device tensors (no host read):
        episodes and timeouts (counts), then means over the finished episodes (divisor max(episodes, 1)): length [policy steps],
        return, displacement [m], level, rew_<term> for the twelve reward terms (unweighted episode sums) and, with tsid,
        teacher_<term>.  One torch.sum over episode_sum; clear: episode_sum is then zeroed, in stream order."""
        if self._episode is None:
            raise _lib.TsidbError("PolicyEnv.episode_stats: the env was built without episode_stats = True or a curriculum")
        s = self.episode_sum.sum(0)
        div = s[_lib.POL_EP_COUNT].clamp(min=1.0)
        out = dict(episodes=s[_lib.POL_EP_COUNT], timeouts=s[_lib.POL_EP_TIMEOUT])
        for k, i in (("length", _lib.POL_EP_LENGTH), ("return", _lib.POL_EP_RETURN), ("displacement", _lib.POL_EP_DISPLACEMENT),
                     ("level", _lib.POL_EP_LEVEL)):
            out[k] = s[i] / div
        for j, k in enumerate(_lib.POL_TERMS):
            out["rew_" + k] = s[_lib.POL_EP_TERMS + j] / div
        if self.tsid is not None:
            for j, k in enumerate(_lib.POL_TEACH_TERMS):
                out["teacher_" + k] = s[_lib.POL_EP_TEACH + j] / div
        if clear:
            self.episode_sum.zero_()
        return out

    def _beta_tensor(self, teacher_beta):
        """teacher_beta as the [1] float32 device tensor the launch reads, or None"""
        wc = self.wc
        if teacher_beta is None:
            return None
        if isinstance(teacher_beta, torch.Tensor):
            if teacher_beta.dtype != torch.float32 or tuple(teacher_beta.shape) != (1,) or teacher_beta.device != wc.device:
                raise _lib.TsidbError(f"PolicyEnv.rollout: a teacher_beta tensor must be [1] float32 on {wc.device}, got "
                                      f"{(tuple(teacher_beta.shape), teacher_beta.dtype, teacher_beta.device)}")
            return teacher_beta
        if isinstance(teacher_beta, bool) or not isinstance(teacher_beta, (int, float)) or not 0 <= teacher_beta <= 1:
            raise _lib.TsidbError(f"PolicyEnv.rollout: teacher_beta must be None, a number in [0, 1] or a [1] float32 tensor, got {teacher_beta!r}")
        if self._teacher_beta is None:
            self._teacher_beta = torch.zeros(1, dtype=torch.float32, device=wc.device)
        self._teacher_beta.fill_(float(teacher_beta))
        return self._teacher_beta

    def _after_reset_done(self, push=1):
        """what reset() and step() launch behind reset_done, each only while its group is on: a new plan, reset noise and new
        tables for the envs just restarted, then the observation, the height scan and the teacher's observation of every env,
        and last the observation history - push = 1 from step(): a new frame for every env; 0 from reset(): only the
        restarted envs are refilled"""
        if self.sched is not None:
            self._replan()
        if self._dr_reset:
            self._reset_noise()
        if self.terrain is not None:
            self._terrain_reset()
        if self._episode is not None:
            self._episode_begin()
        self._obs()
        if self.terrain is not None:
            self._height_scan()
        if self.tsid is not None:
            self._teacher_obs()
        if self._obs_history is not None:
            self._push_obs_history(push)

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
        if self.sched is not None and env_ids is None:
            self.clock.zero_()
        self._after_reset_done(push=0)
        wc.done.zero_()
        self.timeout.zero_()
        return self.obs

    def step(self, action):
        """One policy step for every env; action [N, NA] (self.dtype, on self.device, contiguous) in the actuator order.
        Returns (obs, reward, done, info): views updated in place; info = dict(timeout [N] int32: the episode ended by its
        length alone, terms [N, 12]: the unweighted reward terms, episode_length [N] int32: policy steps into the running
        episode, 0 for an env this step restarted).  obs is the FIRST observation of the new episode for a done env; reward,
        done and terms belong to the step that ended the old one.  With pushes on, info["push"] [N, 3] is the torso force the
        step applied (0 for an env it restarted: the reset clears the wrenches).  With tsid set, info also holds teacher_terms
        [N, 4] (unweighted; already in reward with teacher_weights), teacher_action [N, NA] and teacher_obs [N, 14 + NA].  With
        terrain set, height_scan [N, nx * ny], env_params [N, 8] (the sim's table, as the restarts left it) and terrain_level.
        With episode_stats or a curriculum, episode_last and episode_sum [N, NREC] float64 (see the class).  With obs_history
        set, obs_history [N, frames * K]: the step's observation is its newest frame."""
        wc = self.wc
        if action is None:
            raise _lib.TsidbError("PolicyEnv.step: action is None")
        wc._buffer("PolicyEnv.step", "action", (self.num_envs, self.NA), action)
        self._act(action)
        if self._dr_push:
            self._perturb()
        if self.tsid is None:
            wc.sim_steps(self.decimation)
            self._reward()
        else:
            self._tsid_steps()
            self._reward()
            self._teacher()
        if self._episode is not None:
            self._episode_end()
        wc.reset_done()
        self._after_reset_done()
        info = dict(timeout=self.timeout, terms=self.terms, episode_length=self.ep_len)
        if self._episode is not None:
            info.update(episode_last=self.episode_last, episode_sum=self.episode_sum)
        if self.terrain is not None:
            info.update(height_scan=self.height_scan, env_params=wc.env_params, terrain_level=self.terrain_level)
        if self.tsid is not None:
            info.update(teacher_terms=self.teacher_terms, teacher_action=self.teacher_action, teacher_obs=self.teacher_obs)
        if self._obs_history is not None:
            info["obs_history"] = self.obs_history
        if self._dr_push:
            info["push"] = wc.xfrc[:, 0, :3]
        return self.obs, self.reward, self.done, info

    def rollout(self, actor, steps, storage=None, teacher_beta=None):
        """`steps` policy steps with `actor` (a PolicyActor on this env) in the loop: per step one actor launch - networks, sample,
        log-probability and value on the current observation, written straight into slot t of the storage - then step(action) and
        three device copies of reward, done and timeout; last, one critic-only launch on the final observation into value[steps].
        With a PolicyNormalizer in training mode every step first updates the statistics with its observation; the last launch
        normalises with the statistics as they are and does not update (the next rollout's first step counts that observation).
        storage: a RolloutStorage of this env, actor and length to reuse (None = a new one); returned.  Everything stays on the
        current stream with no host synchronisation, so a whole rollout can be captured in a graph (policy_actor.rollout_written
        lists what it writes beyond written()).  storage.gae(gamma, lam) then gives the advantages and returns.

        With a storage built with teacher = True one more launch per step sits between the actor launch and step()
        (tsidb_policy_teacher_mix): slot t of teacher_action / teacher_weight / teacher_executed gets TSID's label for the stored
        row, its weight (0 for an env the previous step restarted) and whether the env executes the teacher's action - DAgger's
        mixing: for a share teacher_beta of the EPISODES (one draw per env and episode, stream 23 of the randomisation's keys, with
        the actor's seed and env_offset) the teacher's action overwrites the sampled one before the step; storage.action and
        storage.logp stay the policy's own.  teacher_beta: None (no mixing), a number in [0, 1] (kept in a [1] device tensor of
        the env's), or a [1] float32 device tensor of the caller's - read on the device at every launch, so a captured rollout
        follows a beta that a device op decays between replays.  With a plain storage the launches are those above, and
        teacher_beta must be None."""
        from .policy_actor import PolicyActor, RolloutStorage
        if not isinstance(actor, PolicyActor) or actor.env is not self:
            raise _lib.TsidbError("PolicyEnv.rollout: actor must be a PolicyActor built on this env")
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise _lib.TsidbError(f"PolicyEnv.rollout: steps must be a whole number >= 1, got {steps!r}")
        if storage is None:
            storage = RolloutStorage(self, actor, steps)
        elif not isinstance(storage, RolloutStorage) or storage.env is not self or storage.actor is not actor or storage.steps != steps:
            raise _lib.TsidbError("PolicyEnv.rollout: storage must be a RolloutStorage of this env, this actor and this many steps")
        st = storage
        labels = st.teacher_action is not None
        if teacher_beta is not None and not labels:
            raise _lib.TsidbError("PolicyEnv.rollout: teacher_beta needs a storage built with teacher = True (the executed flags are "
                                  "what keeps the surrogate off the teacher's rows)")
        beta = self._beta_tensor(teacher_beta)
        for t in range(steps):
            actor.observe()
            actor._launch(True, action=actor.action, action32=st.action[t], mean=st.mean[t], logp=st.logp[t], value=st.value[t],
                          actor_input=st.actor_input[t], critic_input=st.critic_input[t] if st.critic_input is not None else None)
            if labels:
                self._teacher_mix(actor, actor.action, st.teacher_action[t], st.teacher_weight[t], st.teacher_executed[t], beta)
            self.step(actor.action)
            st.reward[t].copy_(self.reward)
            st.done[t].copy_(self.done)
            st.timeout[t].copy_(self.timeout)
        if actor.critic_net is not None:
            actor._launch(False, actor=False, value=st.value[steps])
        return storage
