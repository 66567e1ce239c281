"""Numpy restatement of the policy environment's randomisation (tsidb_policy_randomize / _perturb / _reset_noise and the
randomised tsidb_policy_obs), written from their description in include/tsidb.h on top of tests/policy_reference.py.  Every
draw is formed in float64 from the hash and cast to `dtype`; the arithmetic around it runs in `dtype`, as there.
tests/test_policy_dr_reference.py pins this module by its properties."""
import numpy as np

from policy_reference import PolicyReference, uniform

# streams of the key layout (include/tsidb.h): key = seed + ((stream * 256 + column) << 32)
S_JOINT_POS, S_JOINT_VEL, S_LIN_VEL, S_ANG_VEL, S_YAW, S_XY, S_OBS, S_PUSH_PHASE, S_PUSH_MAG, S_PUSH_DIR, S_CMD_ZERO = range(1, 12)

FIELDS = dict(seed=0, env_offset=0, reset_joint_pos=0.0, reset_joint_vel=0.0, reset_base_lin_vel=(0.0, 0.0, 0.0),
              reset_base_ang_vel=(0.0, 0.0, 0.0), reset_yaw=0.0, reset_xy=0.0, reset_lift=0.0, noise_ang_vel=0.0, noise_gravity=0.0,
              noise_joint_pos=0.0, noise_joint_vel=0.0, push_interval=0, push_duration=0, push_force_lo=0.0, push_force_hi=0.0,
              command_interval=0, command_zero_prob=0.0)


def key(seed, stream, column=0):
    return int(seed) + ((int(stream) * 256 + int(column)) << 32)


def draw(seed, stream, column, env, counter):
    """U in [0, 1) of (stream, column) for the global env indices `env` and the counters `counter` (uint64 arrays)"""
    return uniform(key(seed, stream, column), env, counter)


def symmetric(seed, stream, column, env, counter, amp):
    """amp (2 U - 1), float64"""
    return float(amp) * (2.0 * draw(seed, stream, column, env, counter) - 1.0)


def counter_hi_lo(hi, lo):
    """hi * 2^32 + lo as uint64"""
    return (np.asarray(hi).astype(np.uint64) << np.uint64(32)) | np.asarray(lo).astype(np.uint64)


def push_force(seed, env, episode, ep_len, interval, duration, lo, hi):
    """(force [n, 3] float64, active [n] bool, k [n]) of the push of the policy step that starts with ep_len completed steps"""
    env, episode, ep_len = (np.atleast_1d(np.asarray(x)).astype(np.int64) for x in (env, episode, ep_len))
    phase = np.floor(draw(seed, S_PUSH_PHASE, 0, env, episode) * interval).astype(np.int64)
    since = ep_len - phase
    k, r = since // interval, since % interval
    active = (since >= 0) & (r < duration)
    ctr = counter_hi_lo(episode, np.where(active, k, 0))
    mag = lo + (hi - lo) * draw(seed, S_PUSH_MAG, 0, env, ctr)
    az = 2.0 * np.pi * draw(seed, S_PUSH_DIR, 0, env, ctr)
    f = np.stack([mag * np.cos(az), mag * np.sin(az), np.zeros_like(mag)], axis=1)
    return np.where(active[:, None], f, 0.0), active, k


def yaw_quat(quat_wxyz, theta, dt=np.float64):
    """(c, 0, 0, s) * quat with c, s = cos, sin(theta / 2) formed in float64 and cast, divided by its norm, in dt"""
    q = np.asarray(quat_wxyz, dtype=dt)
    c, s = np.cos(0.5 * np.asarray(theta, dtype=np.float64)).astype(dt), np.sin(0.5 * np.asarray(theta, dtype=np.float64)).astype(dt)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    out = np.stack([c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w], axis=-1).astype(dt)
    return (out / np.sqrt((out * out).sum(-1, keepdims=True))).astype(dt)


class PolicyDRReference(PolicyReference):
    """PolicyReference plus the randomisation `dr` (a dict over FIELDS; missing = 0)"""

    def __init__(self, *args, dr=None, **kw):
        super().__init__(*args, **kw)
        unknown = set(dr or {}) - set(FIELDS)
        assert not unknown, unknown
        self.dr = dict(FIELDS, **(dr or {}))
        for k in ("reset_base_lin_vel", "reset_base_ang_vel"):
            self.dr[k] = tuple(np.broadcast_to(np.asarray(self.dr[k], dtype=np.float64), (3,)))
        self.genv = np.arange(self.n, dtype=np.int64) + int(self.dr["env_offset"])
        self.resampled, self.zeroed = np.zeros(self.n, bool), np.zeros(self.n, bool)

    # ------------------------------------------------------------------ push (before the sim steps)
    def perturb(self):
        """the torso force [n, 3] of this policy step, and which envs are pushed"""
        d = self.dr
        f, active, _ = push_force(d["seed"], self.genv, self.episode, self.ep_len, int(d["push_interval"]), int(d["push_duration"]),
                                  d["push_force_lo"], d["push_force_hi"])
        return f.astype(self.dt), active

    # ------------------------------------------------------------------ reset noise (after the reset, before obs_stage)
    def reset_noise(self, done, qpos, qvel):
        """qpos, qvel of the reset state with the noise of the envs whose done flag is set"""
        d, dt, seed = self.dr, self.dt, self.dr["seed"]
        fresh = np.asarray(done) != 0
        ep = (self.episode + 1).astype(np.int64)       # the episode about to start
        qp, qv = np.array(qpos, dtype=dt), np.array(qvel, dtype=dt)
        new_qp, new_qv = qp.copy(), qv.copy()
        for a, dof in enumerate(self.act_dof):
            if d["reset_joint_pos"] != 0:
                new_qp[:, dof + 1] = qp[:, dof + 1] + symmetric(seed, S_JOINT_POS, a, self.genv, ep, d["reset_joint_pos"]).astype(dt)
            if d["reset_joint_vel"] != 0:
                new_qv[:, dof] = qv[:, dof] + symmetric(seed, S_JOINT_VEL, a, self.genv, ep, d["reset_joint_vel"]).astype(dt)
        for i in range(3):
            if d["reset_base_lin_vel"][i] != 0:
                new_qv[:, i] = qv[:, i] + symmetric(seed, S_LIN_VEL, i, self.genv, ep, d["reset_base_lin_vel"][i]).astype(dt)
            if d["reset_base_ang_vel"][i] != 0:
                new_qv[:, 3 + i] = qv[:, 3 + i] + symmetric(seed, S_ANG_VEL, i, self.genv, ep, d["reset_base_ang_vel"][i]).astype(dt)
        if d["reset_xy"] != 0:
            for i in range(2):
                new_qp[:, i] = qp[:, i] + symmetric(seed, S_XY, i, self.genv, ep, d["reset_xy"]).astype(dt)
        if d["reset_lift"] != 0:
            new_qp[:, 2] = qp[:, 2] + dt(d["reset_lift"])
        if d["reset_yaw"] != 0:
            new_qp[:, 3:7] = yaw_quat(qp[:, 3:7], symmetric(seed, S_YAW, 0, self.genv, ep, d["reset_yaw"]), dt)
        return np.where(fresh[:, None], new_qp, qp), np.where(fresh[:, None], new_qv, qv)

    # ------------------------------------------------------------------ obs (commands, noise)
    def obs_stage(self, done, qpos, qvel, ncon, con_pairs):
        d, dt, na, seed = self.dr, self.dt, self.na, self.dr["seed"]
        fresh = np.asarray(done) != 0
        before = self.command.copy()
        o = super().obs_stage(done, qpos, qvel, ncon, con_pairs)   # (bookkeeping; its command draw ignores env_offset: redone here)
        ci = int(d["command_interval"])
        resample = ~fresh & (ci > 0) & (self.ep_len > 0) & (self.ep_len % max(ci, 1) == 0)
        event = fresh | resample
        k = np.where(resample, self.ep_len // max(ci, 1), 0).astype(np.uint64)
        ctr = self.episode.astype(np.uint64) + (k << np.uint64(32))
        zero = event & (d["command_zero_prob"] > 0) & (draw(seed, S_CMD_ZERO, 0, self.genv, ctr) < d["command_zero_prob"])
        cmd = before
        for i in range(3):
            if self.cmd_lo[i] != self.cmd_hi[i]:
                new = (self.cmd_lo[i] + (self.cmd_hi[i] - self.cmd_lo[i]) * uniform(self.seed + i, self.genv, ctr)).astype(dt)
                cmd[:, i] = np.where(event, new, cmd[:, i])
        cmd[zero] = 0
        self.command, self.resampled, self.zeroed = cmd, resample, zero
        o[:, 6:9] = cmd
        nctr = counter_hi_lo(self.episode, self.ep_len)
        for cols, amp in ((range(0, 3), d["noise_ang_vel"]), (range(3, 6), d["noise_gravity"]), (range(9, 9 + na), d["noise_joint_pos"]),
                          (range(9 + na, 9 + 2 * na), d["noise_joint_vel"])):
            if amp != 0:
                for j in cols:
                    o[:, j] = o[:, j] + symmetric(seed, S_OBS, j, self.genv, nctr, amp).astype(dt)
        self.obs = o
        return o
