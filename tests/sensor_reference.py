"""Independent float64 restatement of the sim stage's site sensors (tsidb_set_sensors; MuJoCo's mj_data.sensordata as
mj_sensorPos / mj_sensorVel / mj_sensorAcc fill it): from the blob's mj_* sections, the qpos / qvel a step starts from and
the qacc it solves for, the 22 values per site by the textbook body-by-body recursion on CLASSICAL quantities - position,
rotation, angular velocity, velocity and acceleration of each body's own origin, all in the world frame.  Nothing of the
kernel's formulation is used (spatial vectors about a common origin, bias acceleration plus S qacc).

Row layout (include/tsidb.h): framepos 0-2, framequat 3-6 (wxyz), framelinvel 7-9, frameangvel 10-12, velocimeter 13-15,
gyro 16-18, accelerometer 19-21.  tests/test_sensor_reference.py pins this module by finite differences and closed forms."""
import numpy as np

COLS = dict(framepos=slice(0, 3), framequat=slice(3, 7), framelinvel=slice(7, 10), frameangvel=slice(10, 13),
            velocimeter=slice(13, 16), gyro=slice(16, 19), accelerometer=slice(19, 22))
NVAL = 22


def quat_to_mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mat_to_quat(R):
    """wxyz, unit; the component with the largest magnitude is taken from a square root (stable at every angle); the sign
    is the one that makes that component positive - compare quaternions up to sign (q and -q are one orientation)"""
    d = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(d))
    if k == 0:
        s = 2 * np.sqrt(1 + d[0])
        q = np.array([s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = k - 1
        j, l = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[l, l])
        q = np.zeros(4)
        q[0] = (R[l, j] - R[j, l]) / s
        q[1 + i] = s / 4
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + l] = (R[l, i] + R[i, l]) / s
    return q / np.linalg.norm(q)


def exp_so3(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


class FK:
    """The sim tree of the blob's mj_* sections: R_b = R_parent mj_R[b] Rz(theta_b), p_b = p_parent + R_parent pos_b
    (body 0 = the torso with the free joint: position qpos[:3], quaternion qpos[3:7] wxyz; body b > 0 hangs on a hinge
    about its own z axis through its own origin, angle qpos[6 + b])."""

    def __init__(self, blob):
        self.NB = int(blob["model_dims"][4])
        self.parent = blob["mj_parent"].copy()
        self.pos = blob["mj_pos"].reshape(self.NB, 3)
        self.Rq = np.stack([quat_to_mat(q) for q in blob["mj_quat"].reshape(self.NB, 4)])
        self.gz = float(blob["mj_opt"][1])

    def run(self, qpos, R0=None):
        R, p = np.zeros((self.NB, 3, 3)), np.zeros((self.NB, 3))
        R[0] = quat_to_mat(qpos[3:7]) if R0 is None else R0
        p[0] = qpos[:3]
        for b in range(1, self.NB):
            a = self.parent[b]
            c, s = np.cos(qpos[6 + b]), np.sin(qpos[6 + b])
            R[b] = R[a] @ self.Rq[b] @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
            p[b] = p[a] + R[a] @ self.pos[b]
        return R, p

    def site_pose(self, qpos, sites, R0=None):
        """world position [S, 3] and rotation [S, 3, 3] of each site (body, pos, quat)"""
        R, p = self.run(qpos, R0)
        P = np.stack([p[b] + R[b] @ np.asarray(ps, dtype=np.float64) for b, ps, _ in sites])
        Rs = np.stack([R[b] @ quat_to_mat(qs) for b, _, qs in sites])
        return P, Rs

    def moved(self, qpos, dq):
        """q (+) dq: (qpos', R0') with the free joint's rotation R exp([dq[3:6]]) (body-frame increment)"""
        q = np.array(qpos, dtype=np.float64)
        q[:3] += dq[:3]
        q[7:] += dq[6:]
        return q, quat_to_mat(qpos[3:7]) @ exp_so3(dq[3:6])


def sensors(blob, qpos, qvel, qacc, sites, fk=None):
    """[S, 22] sensor values of the sites (body, pos [3], quat [4] wxyz) for one env: qpos [NQ], qvel [NV] at the start of
    the step, qacc [NV] the step's acceleration (qvel[:3] world-frame linear, qvel[3:6] body-frame angular)."""
    fk = fk or FK(blob)
    qpos, qvel, qacc = (np.asarray(x, dtype=np.float64) for x in (qpos, qvel, qacc))
    NB = fk.NB
    R, p = fk.run(qpos)
    w, v, al, a = (np.zeros((NB, 3)) for _ in range(4))
    v[0], a[0] = qvel[:3], qacc[:3]
    w[0], al[0] = R[0] @ qvel[3:6], R[0] @ qacc[3:6]     # d/dt (R w_l) = R dw_l + R (w_l x w_l)
    for b in range(1, NB):
        pa = fk.parent[b]
        d = p[b] - p[pa]                                  # fixed in the parent
        z = R[b][:, 2]                                    # hinge axis; dz/dt = w_parent x z
        v[b] = v[pa] + np.cross(w[pa], d)
        a[b] = a[pa] + np.cross(al[pa], d) + np.cross(w[pa], np.cross(w[pa], d))
        w[b] = w[pa] + z * qvel[5 + b]
        al[b] = al[pa] + z * qacc[5 + b] + np.cross(w[pa], z) * qvel[5 + b]
    g = np.array([0.0, 0.0, fk.gz])
    out = np.zeros((len(sites), NVAL))
    for i, (b, ps, qs) in enumerate(sites):
        r = R[b] @ np.asarray(ps, dtype=np.float64)
        Rs = R[b] @ quat_to_mat(qs)
        vs = v[b] + np.cross(w[b], r)
        acc = a[b] + np.cross(al[b], r) + np.cross(w[b], np.cross(w[b], r))
        out[i, 0:3] = p[b] + r
        out[i, 3:7] = mat_to_quat(Rs)
        out[i, 7:10], out[i, 10:13] = vs, w[b]
        out[i, 13:16], out[i, 16:19] = Rs.T @ vs, Rs.T @ w[b]
        out[i, 19:22] = Rs.T @ (acc - g)
    return out


def align_quat(got, want):
    """`want` [..., 4] with the sign of each quaternion chosen as in `got` (q and -q are the same orientation, and which
    of them a four-case conversion returns depends on the case it takes)"""
    s = np.sign(np.sum(got * want, axis=-1, keepdims=True))
    return want * np.where(s == 0, 1.0, s)


def site_jacobian_acc(blob, qpos, qacc, sites, fk=None):
    """[S, 3] world-frame J_site qacc: the part of the site's linear acceleration that is linear in qacc (zero velocity)"""
    fk = fk or FK(blob)
    z = np.zeros(len(qacc))
    g0 = sensors(blob, qpos, z, z, sites, fk)
    g1 = sensors(blob, qpos, z, qacc, sites, fk)
    _, Rs = fk.site_pose(qpos, sites)
    return np.einsum("sij,sj->si", Rs, g1[:, 19:22] - g0[:, 19:22])
