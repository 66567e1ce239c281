"""Numpy restatement of the two kernels that put TSID into the policy environment's loop (tsidb_policy_teacher /
tsidb_policy_teacher_obs), written from their description in include/tsidb.h, vectorised over the envs.  Arithmetic runs in
`dtype`, as in tests/policy_reference.py: float64 is the reference the device is compared with, the same code in float32
measures what float32 arithmetic costs on given states.  Nothing here keeps state: every call takes the device's own buffers
and returns what the kernel leaves in them.  tests/test_policy_teacher_reference.py pins this module by hand-made states."""
import numpy as np

from policy_reference import rot_rows

TEACH_TERMS = ("track_com", "track_feet", "contact_match", "deviation")
TEACH_NT = 4
TERMINATION = 11          # the termination term's column of the reward terms (tests/policy_reference.py TERMS)


def foot_contacts(ncon, con_pairs, geom_body, foot_bodies):
    """[n, 2] bool: a live floor row of the contact list on a geom of each sole body"""
    geom_body = np.asarray(geom_body, dtype=np.int64)
    cp = np.asarray(con_pairs, dtype=np.int64)
    row = np.arange(cp.shape[1])[None, :] < np.asarray(ncon)[:, None]
    live = row & (cp >= 0) & ((cp & 0x8000) == 0)
    g = np.where(live, cp >> 16, 0)
    live &= g < len(geom_body)
    body = geom_body[np.where(live, g, 0)]
    return np.stack([(live & (body == int(b))).any(1) for b in foot_bodies], axis=1)


class TeacherReference:
    """ctrl_qidx [na]: index into the TSID q of each actuator's joint (its tau is tau[ctrl_qidx - 7]); nq, nv: sizes of the
    TSID state, which place com / LF / RF in the tick's row (q v com cop LF RF); mode: "residual", "motor" or "position";
    term_weight: the termination weight of the reward."""

    def __init__(self, ctrl_qidx, geom_body, foot_bodies, scale, default, *, nq, nv, clip=100.0, mode="residual", sigma_com=0.05,
                 sigma_foot=0.05, weights=None, term_weight=0.0, dtype=np.float64):
        self.dt = dt = np.dtype(dtype).type
        self.qidx = np.asarray(ctrl_qidx, dtype=np.int64)
        self.na = len(self.qidx)
        self.geom_body, self.foot_bodies = np.asarray(geom_body, dtype=np.int64), tuple(int(b) for b in foot_bodies)
        self.scale, self.default = np.asarray(scale, dtype=np.float64).astype(dt), np.asarray(default, dtype=np.float64).astype(dt)
        self.clip, self.sigma_com, self.sigma_foot, self.term_weight = dt(clip), dt(sigma_com), dt(sigma_foot), dt(term_weight)
        assert mode in ("residual", "motor", "position")
        self.mode = mode
        w = np.zeros(TEACH_NT)
        for k, v in (weights or {}).items():
            w[TEACH_TERMS.index(k)] = v
        self.w = w.astype(dt)
        self.com0, self.lf0, self.rf0 = nq + nv, nq + nv + 6, nq + nv + 9
        self.nobs = nq + nv + 12

    def tau_act(self, tau):
        """tau in the actuator order"""
        return np.asarray(tau, dtype=self.dt)[:, self.qidx - 7]

    # ------------------------------------------------------------------ after the reward, before the reset
    def teacher(self, rows, q, tau, status, ctrl, ncon, con_pairs, com_ref, foot_ref, contact_active, reward, done, timeout, terms):
        """reward, done [n], timeout [n] int, terms [n, 12]: as the reward stage left them.  Returns dict(teacher_terms [n, 4],
        teacher_action [n, na], reward, done, timeout, terms) as the kernel leaves them."""
        dt = self.dt
        rows, com_ref = np.asarray(rows, dtype=dt), np.asarray(com_ref, dtype=dt)
        foot_ref = np.asarray(foot_ref, dtype=dt).reshape(len(rows), 2, 24)
        ctrl, ta, q = np.asarray(ctrl, dtype=dt), self.tau_act(tau), np.asarray(q, dtype=dt)
        ec = ((rows[:, self.com0:self.com0 + 3] - com_ref[:, 0:3]) ** 2).sum(1)
        ef = ((rows[:, self.lf0:self.lf0 + 3] - foot_ref[:, 0, 0:3]) ** 2).sum(1) + ((rows[:, self.rf0:self.rf0 + 3] - foot_ref[:, 1, 0:3]) ** 2).sum(1)
        foot = foot_contacts(ncon, con_pairs, self.geom_body, self.foot_bodies)
        active = np.asarray(contact_active).reshape(len(rows), 2) != 0
        t = np.zeros((len(rows), TEACH_NT), dtype=dt)
        t[:, 0] = np.exp(-ec / (self.sigma_com * self.sigma_com))
        t[:, 1] = np.exp(-ef / (self.sigma_foot * self.sigma_foot))
        t[:, 2] = (foot == active).sum(1)
        if self.mode == "residual":
            t[:, 3] = (ctrl ** 2).sum(1)
        elif self.mode == "motor":
            t[:, 3] = ((ctrl - ta) ** 2).sum(1)
        add = np.zeros(len(rows), dtype=dt)
        with np.errstate(invalid="ignore"):
            for k in range(TEACH_NT):
                add = (add + self.w[k] * t[:, k]).astype(dt)
        rew = (np.asarray(reward, dtype=dt) + add).astype(dt)
        terms = np.array(terms, dtype=dt)
        failed = np.asarray(status) != 0
        newly = failed & (terms[:, TERMINATION] == 0)
        rew = np.where(newly, rew + self.term_weight, rew).astype(dt)
        terms[:, TERMINATION] = np.where(failed, dt(1), terms[:, TERMINATION])
        done = np.where(failed, dt(1), np.asarray(done, dtype=dt))
        timeout = np.where(failed, 0, np.asarray(timeout)).astype(np.int32)
        act = np.zeros((len(rows), self.na), dtype=dt)
        if self.mode != "residual":
            cmd = ta if self.mode == "motor" else q[:, self.qidx]
            on = self.scale != 0
            with np.errstate(invalid="ignore", divide="ignore"):
                a = (cmd - self.default) / np.where(on, self.scale, dt(1))
            a = np.where(a > self.clip, self.clip, np.where(a < -self.clip, -self.clip, a))
            act = np.where(on[None, :], a, dt(0)).astype(dt)
        return dict(teacher_terms=t, teacher_action=act, reward=rew, done=done, timeout=timeout, terms=terms)

    # ------------------------------------------------------------------ after the observation
    def teacher_obs(self, done, rows, qpos, tau, com_ref, foot_ref, contact_active):
        """done: the flags the reset acted on; rows: the last tick's; qpos, com_ref, foot_ref, contact_active: AFTER the reset"""
        dt, n = self.dt, len(rows)
        rows, com_ref, qp = np.asarray(rows, dtype=dt), np.asarray(com_ref, dtype=dt), np.asarray(qpos, dtype=dt)
        foot_ref = np.asarray(foot_ref, dtype=dt).reshape(n, 2, 24)
        fresh = np.asarray(done) != 0
        R = rot_rows(qp[:, 3:7], dt)
        body = lambda w: np.einsum("nji,nj->ni", R, w).astype(dt)      # R^T w
        keep = (~fresh)[:, None]
        o = np.zeros((n, 14 + self.na), dtype=dt)
        o[:, 0:2] = np.asarray(contact_active).reshape(n, 2) != 0
        o[:, 2:5] = np.where(keep, body(com_ref[:, 0:3] - rows[:, self.com0:self.com0 + 3]), dt(0))
        o[:, 5:8] = body(com_ref[:, 3:6])
        o[:, 8:11] = np.where(keep, body(foot_ref[:, 0, 0:3] - rows[:, self.lf0:self.lf0 + 3]), dt(0))
        o[:, 11:14] = np.where(keep, body(foot_ref[:, 1, 0:3] - rows[:, self.rf0:self.rf0 + 3]), dt(0))
        o[:, 14:] = np.where(keep, self.tau_act(tau), dt(0))
        return o
