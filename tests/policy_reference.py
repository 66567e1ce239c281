"""Numpy restatement of the policy environment's three kernels (tsidb_policy_act / _reward / _obs), written from their
description in include/tsidb.h, vectorised over the envs.  Arithmetic runs in `dtype`: float64 is the reference the device is
compared with; the same code in float32 measures what float32 arithmetic costs on given states (the float32 gates of
tests/test_gpu_policy_env.py).  plan_hash is the device's SplitMix64 of (seed, env, episode) in uint64.
tests/test_policy_reference.py pins this module by closed forms and invariances."""
import numpy as np

TERMS = ("track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "action_rate",
         "joint_vel", "feet_air_time", "alive", "termination")
NT, HIST, NPRIV = 12, 8, 4


def plan_hash(seed, env, episode):
    """uint64 arrays (or scalars) -> uint64 array"""
    u = lambda x: np.atleast_1d(np.asarray(x)).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = u(seed) ^ (u(env) * np.uint64(0x9E3779B97F4A7C15)) ^ (u(episode) * np.uint64(0xD1B54A32D192ED03))
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform(seed, env, episode):
    """[0, 1): the top 53 bits of the hash over 2^53"""
    return (plan_hash(seed, env, episode) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def rot_rows(quat_wxyz, dt):
    """[n, 3, 3] rotation of each (normalised) wxyz quaternion"""
    q = np.asarray(quat_wxyz, dtype=dt)
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = dt(1), dt(2)
    R = np.empty((len(q), 3, 3), dtype=dt)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
    return R


class PolicyReference:
    """State and the three stages for n envs of a robot with na actuators.  act_dof [na]: dof of each actuator (qvel index;
    qpos index + 1); geom_body [ng]: sim body of each collision geom; foot_bodies (2): the sole bodies LF, RF."""

    def __init__(self, n, act_dof, geom_body, foot_bodies, scale, default, *, clip=100.0, alpha=1.0, sigma=0.25, h_target=0.33,
                 t_air=0.25, deadband=0.1, max_episode_steps=0, decimation=10, sim_dt=0.002, seed=0, cmd_lo=(0, 0, 0), cmd_hi=(0, 0, 0),
                 weights=None, term_body_mask=1, done_height=0.2, done_tilt=np.cos(np.deg2rad(45.0)), position_mode=True,
                 dtype=np.float64):
        self.dt = dt = np.dtype(dtype).type
        self.n, self.na = n, len(act_dof)
        self.act_dof, self.geom_body = np.asarray(act_dof, dtype=np.int64), np.asarray(geom_body, dtype=np.int64)
        self.foot_bodies = tuple(int(b) for b in foot_bodies)
        self.scale, self.default = np.asarray(scale, dtype=np.float64).astype(dt), np.asarray(default, dtype=np.float64).astype(dt)
        self.clip, self.alpha, self.sigma, self.h_target, self.t_air, self.deadband = (dt(v) for v in (clip, alpha, sigma, h_target, t_air, deadband))
        self.air_dt = dt(decimation * sim_dt)
        self.done_height, self.done_tilt = dt(done_height), dt(done_tilt)
        self.max_episode_steps, self.seed = int(max_episode_steps), int(seed)
        self.cmd_lo, self.cmd_hi = np.asarray(cmd_lo, dtype=np.float64), np.asarray(cmd_hi, dtype=np.float64)
        w = np.zeros(NT)
        for k, v in (weights or {}).items():
            w[TERMS.index(k)] = v
        self.w = w.astype(dt)
        self.term_body_mask, self.position_mode = int(term_body_mask), bool(position_mode)
        na = self.na
        self.nobs = 11 + 3 * na
        z = lambda *s: np.zeros(s, dtype=dt)
        self.hist, self.last, self.prev, self.ctrl = z(HIST, n, na), z(n, na), z(n, na), z(n, na)
        self.command, self.air, self.terms, self.reward, self.done = z(n, 3), z(n, 2), z(n, NT), z(n), z(n)
        self.command[:] = self.cmd_lo.astype(dt)
        self.ep_len, self.episode, self.timeout = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.delay = np.zeros(n, np.int32)
        self.obs = z(n, self.nobs + NPRIV)

    # ------------------------------------------------------------------ contacts
    def contact_flags(self, ncon, con_pairs):
        """(foot [n, 2] bool, term [n] bool): a live floor row on a geom of each sole body / of a body of the mask"""
        cp = np.asarray(con_pairs, dtype=np.int64)
        row = np.arange(cp.shape[1])[None, :] < np.asarray(ncon)[:, None]
        live = row & (cp >= 0) & ((cp & 0x8000) == 0)
        g = np.where(live, cp >> 16, 0)
        live &= g < len(self.geom_body)
        body = self.geom_body[np.where(live, g, 0)]
        foot = np.stack([(live & (body == b)).any(1) for b in self.foot_bodies], axis=1)
        term = (live & (((self.term_body_mask >> body) & 1) != 0)).any(1)
        return foot, term

    # ------------------------------------------------------------------ act
    def act(self, action):
        dt, e = self.dt, np.arange(self.n)
        a = np.asarray(action, dtype=dt)
        act = np.where(a > self.clip, self.clip, np.where(a < -self.clip, -self.clip, a)).astype(dt)   # NaN passes
        self.hist[self.ep_len & 7, e] = act
        d = np.clip(self.delay, 0, HIST - 1)
        delayed = self.hist[(self.ep_len - d) & 7, e]
        delayed = np.where((d > self.ep_len)[:, None], dt(0), delayed)
        target = (self.default + self.scale * delayed).astype(dt)
        self.ctrl = target if self.alpha == dt(1) else (self.ctrl + self.alpha * (target - self.ctrl)).astype(dt)
        self.prev = self.last
        self.last = act
        return self.ctrl

    # ------------------------------------------------------------------ reward
    def reward_stage(self, qpos, qvel, ncon, con_pairs, info, act_force=None):
        dt = self.dt
        qp, qv = np.asarray(qpos, dtype=dt), np.asarray(qvel, dtype=dt)
        R = rot_rows(qp[:, 3:7], dt)
        v = np.einsum("nji,nj->ni", R, qv[:, 0:3]).astype(dt)     # R^T v
        om = qv[:, 3:6]
        cmd = self.command
        foot, term_con = self.contact_flags(ncon, con_pairs)
        s2 = self.sigma * self.sigma
        t = np.zeros((self.n, NT), dtype=dt)
        t[:, 0] = np.exp(-((cmd[:, 0] - v[:, 0]) ** 2 + (cmd[:, 1] - v[:, 1]) ** 2) / s2)
        t[:, 1] = np.exp(-((cmd[:, 2] - om[:, 2]) ** 2) / s2)
        t[:, 2] = v[:, 2] ** 2
        t[:, 3] = om[:, 0] ** 2 + om[:, 1] ** 2
        t[:, 4] = R[:, 2, 0] ** 2 + R[:, 2, 1] ** 2                # g = -R[2, :]
        t[:, 5] = (qp[:, 2] - self.h_target) ** 2
        t[:, 6] = 0 if act_force is None else (np.asarray(act_force, dtype=dt) ** 2).sum(1)
        t[:, 7] = ((self.last - self.prev) ** 2).sum(1)
        t[:, 8] = (qv[:, self.act_dof] ** 2).sum(1)
        moving = np.sqrt(cmd[:, 0] ** 2 + cmd[:, 1] ** 2) > self.deadband
        first = foot & (self.air > 0)
        t[:, 9] = (np.where(first, self.air - self.t_air, dt(0)).sum(1) * moving).astype(dt)
        t[:, 10] = 1
        finite = np.isfinite(qp).all(1) & np.isfinite(qv).all(1)
        up = dt(1) - dt(2) * (qp[:, 4] * qp[:, 4] + qp[:, 5] * qp[:, 5])
        terminated = ((np.asarray(info)[:, 3] & 4) != 0) | ~finite | (qp[:, 2] < self.done_height) | (up < self.done_tilt) | term_con
        t[:, 11] = terminated
        timeout = ~terminated & (self.max_episode_steps > 0) & (self.ep_len + 1 >= self.max_episode_steps)
        rew = np.zeros(self.n, dtype=dt)
        with np.errstate(invalid="ignore"):              # (a non-finite state: 0 * inf, as on the device)
            for k in range(NT):
                rew = (rew + self.w[k] * t[:, k]).astype(dt)
        self.air = np.where(foot, dt(0), self.air + self.air_dt).astype(dt)
        self.terms, self.reward = t, rew
        self.done = (terminated | timeout).astype(dt)
        self.timeout = timeout.astype(np.int32)
        self.ep_len = self.ep_len + 1
        return rew, self.done

    # ------------------------------------------------------------------ obs
    def obs_stage(self, done, qpos, qvel, ncon, con_pairs):
        """done: the flags the reset acted on; qpos / qvel: the state AFTER the reset"""
        dt, na = self.dt, self.na
        fresh = np.asarray(done) != 0
        self.hist[:, fresh] = 0
        self.last = np.where(fresh[:, None], dt(0), self.last)
        self.prev = np.where(fresh[:, None], dt(0), self.prev)
        self.air = np.where(fresh[:, None], dt(0), self.air)
        self.ep_len = np.where(fresh, 0, self.ep_len).astype(np.int32)
        self.ctrl = np.where(fresh[:, None], self.default[None, :] if self.position_mode else dt(0), self.ctrl).astype(dt)
        self.episode = (self.episode + fresh).astype(np.int32)
        for i in range(3):
            if self.cmd_lo[i] != self.cmd_hi[i]:
                u = uniform(self.seed + i, np.arange(self.n), self.episode)
                new = (self.cmd_lo[i] + (self.cmd_hi[i] - self.cmd_lo[i]) * u).astype(dt)
                self.command[:, i] = np.where(fresh, new, self.command[:, i])
        qp, qv = np.asarray(qpos, dtype=dt), np.asarray(qvel, dtype=dt)
        R = rot_rows(qp[:, 3:7], dt)
        foot, _ = self.contact_flags(ncon, con_pairs)
        foot = foot | fresh[:, None]
        o = np.zeros((self.n, self.nobs + NPRIV), dtype=dt)
        o[:, 0:3] = qv[:, 3:6]
        o[:, 3:6] = -R[:, 2, :]
        o[:, 6:9] = self.command
        o[:, 9:9 + na] = qp[:, self.act_dof + 1] - self.default
        o[:, 9 + na:9 + 2 * na] = qv[:, self.act_dof]
        o[:, 9 + 2 * na:9 + 3 * na] = self.last
        o[:, 9 + 3 * na:11 + 3 * na] = foot
        o[:, self.nobs:self.nobs + 3] = np.einsum("nji,nj->ni", R, qv[:, 0:3])
        o[:, self.nobs + 3] = qp[:, 2]
        self.obs = o
        return o
