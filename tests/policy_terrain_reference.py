"""Numpy restatement of the policy environment's per-episode terrain and dynamics and of its height scan
(tsidb_policy_terrain_reset / tsidb_policy_height_scan), written from their description in include/tsidb.h.  The hash and the
key layout are those of tests/policy_dr_reference.py.  Every drawn value is formed in float64 and cast to `dtype`; the scan's
arithmetic runs in `dtype`.  The cell of a point comes from np.floor here, not from the device's helper.
tests/test_policy_terrain_reference.py pins this module by its properties."""
import numpy as np

from policy_dr_reference import counter_hi_lo, draw

# streams 12 .. 20 of the key layout (include/tsidb.h): key = seed + ((stream * 256 + column) << 32)
S_MASS, S_FRICTION, S_TILT, S_AZIMUTH, S_DIRECTION, S_LENGTH, S_RAISED, S_HEIGHT, S_SCAN = range(12, 21)

FIELDS = dict(seed=0, env_offset=0, mass=(1.0, 1.0), friction=(1.0, 1.0), tilt_max=0.0, step_height=(0.0, 0.0), step_length=(0.08, 0.08),
              step_prob=0.5, flat_cells=1, num_levels=1, scan_x=None, scan_y=None, scan_clip=(-1.0, 1.0), scan_noise=0.0)


def nominal_tables(n, dtype=np.float64):
    """(env_params [n, 8], terrain [n, 20]) of the nominal model: mass scale and friction 1, floor z = 0, level, 1 / L = 1"""
    ep, tr = np.zeros((n, 8), dtype=dtype), np.zeros((n, 20), dtype=dtype)
    ep[:, 0] = ep[:, 1] = ep[:, 4] = 1
    tr[:, 3] = 1
    return ep, tr


class PolicyTerrainReference:
    """cfg: a dict over FIELDS (tilt_max in rad; scan_x / scan_y = (first, last, points) or None; missing = the default)"""

    def __init__(self, n, cfg=None, dtype=np.float64):
        unknown = set(cfg or {}) - set(FIELDS)
        assert not unknown, unknown
        self.cfg = dict(FIELDS, **(cfg or {}))
        self.n, self.dt = n, np.dtype(dtype).type
        self.genv = np.arange(n, dtype=np.int64) + int(self.cfg["env_offset"])
        self.env_params, self.terrain = nominal_tables(n, dtype)
        self.raised = np.zeros((n, 16), bool)

    # ------------------------------------------------------------------ restart rows
    def rows(self, episode_next, xb, yb, level=None):
        """(env_params [n, 8], terrain [n, 20], raised [n, 16]) every env would get at the start of episode_next [n], standing at
        (xb, yb) [n]; float64, uncast"""
        c, seed, env = self.cfg, self.cfg["seed"], self.genv
        ep = np.asarray(episode_next).astype(np.int64)
        xb, yb = np.asarray(xb, dtype=np.float64), np.asarray(yb, dtype=np.float64)
        u = lambda stream, column=0: draw(seed, stream, column, env, ep)
        nl = int(c["num_levels"])
        lvl = np.full(self.n, nl - 1) if level is None else np.clip(np.asarray(level).astype(np.int64), 0, nl - 1)
        mass = c["mass"][0] + (c["mass"][1] - c["mass"][0]) * u(S_MASS)
        fric = c["friction"][0] + (c["friction"][1] - c["friction"][0]) * u(S_FRICTION)
        t, a, g = c["tilt_max"] * u(S_TILT), 2.0 * np.pi * u(S_AZIMUTH), 2.0 * np.pi * u(S_DIRECTION)
        length = c["step_length"][0] + (c["step_length"][1] - c["step_length"][0]) * u(S_LENGTH)
        H = (c["step_height"][0] + (c["step_height"][1] - c["step_height"][0]) * u(S_HEIGHT)) * (lvl + 1) / nl
        nx, ny, nz = np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)
        envp = np.zeros((self.n, 8))
        envp[:, 0], envp[:, 1], envp[:, 2], envp[:, 3], envp[:, 4], envp[:, 5] = mass, fric, nx, ny, nz, nx * xb + ny * yb
        terr = np.zeros((self.n, 20))
        terr[:, 0], terr[:, 1], terr[:, 3] = np.cos(g), np.sin(g), 1.0 / length
        terr[:, 2] = np.cos(g) * xb + np.sin(g) * yb - 0.5 * length
        cells = np.arange(16)
        raised = np.stack([u(S_RAISED, k) < c["step_prob"] for k in cells], axis=1)
        raised &= ((cells > c["flat_cells"]) & (cells < 16 - c["flat_cells"]))[None, :]
        terr[:, 4:] = np.where(raised, H[:, None], 0.0)
        return envp, terr, raised

    def reset(self, done, episode, qpos, level=None):
        """rewrites the rows of the envs whose done flag is set; episode [n] as it is BEFORE tsidb_policy_obs increments it,
        qpos [n, >= 2] the state the reset and its noise left.  Returns which rows were rewritten"""
        fresh = np.asarray(done) != 0
        qp = np.asarray(qpos)
        envp, terr, raised = self.rows(np.asarray(episode).astype(np.int64) + 1, qp[:, 0], qp[:, 1], level)
        self.env_params = np.where(fresh[:, None], envp.astype(self.dt), self.env_params)
        self.terrain = np.where(fresh[:, None], terr.astype(self.dt), self.terrain)
        self.raised = np.where(fresh[:, None], raised, self.raised)
        return fresh

    # ------------------------------------------------------------------ height scan
    def points(self):
        """(px [np], py [np]) of the grid in the heading frame, point p = ix * ny + iy; float64"""
        sx, sy = self.cfg["scan_x"], self.cfg["scan_y"]
        if sx is None or sy is None:
            return np.zeros(0), np.zeros(0)
        axis = lambda first, last, k: np.full(1, float(first)) if int(k) == 1 else first + (last - first) * np.arange(int(k)) / (int(k) - 1)
        ax, ay = axis(*sx), axis(*sy)
        return np.repeat(ax, len(ay)), np.tile(ay, len(ax))

    def scan(self, qpos, episode=None, ep_len=None, tables=True):
        """(scan [n, np] in dtype, frac [n, np] float64 = (direction . (X, Y) - phase) / L, over [n, np] = the strip's height
        under the point); episode, ep_len as tsidb_policy_obs leaves them (needed with scan_noise only).  tables = False: no
        table registered, the nominal floor"""
        dt, c = self.dt, self.cfg
        qp = np.asarray(qpos).astype(dt)
        envp, terr = (self.env_params, self.terrain) if tables else nominal_tables(self.n, dt)
        px64, py64 = self.points()
        px, py = px64.astype(dt)[None, :], py64.astype(dt)[None, :]
        w, x, y, z = (qp[:, 3 + i][:, None] for i in range(4))
        hx, hy = dt(1) - dt(2) * (y * y + z * z), dt(2) * (w * z + x * y)
        h2 = hx * hx + hy * hy
        small = h2 < dt(1e-12)
        with np.errstate(invalid="ignore", divide="ignore"):
            hn = np.sqrt(h2)
            hx, hy = np.where(small, dt(1), hx / hn), np.where(small, dt(0), hy / hn)
        X, Y = qp[:, 0:1] + (hx * px - hy * py), qp[:, 1:2] + (hy * px + hx * py)
        u = terr[:, 0:1] * X + terr[:, 1:2] * Y
        frac = (u - terr[:, 2:3]) * terr[:, 3:4]
        with np.errstate(invalid="ignore"):
            cell = np.floor(frac).astype(np.int64) & 15
        over = np.take_along_axis(terr[:, 4:], cell, axis=1)
        zs = (envp[:, 5:6] + over - envp[:, 2:3] * X - envp[:, 3:4] * Y) / envp[:, 4:5]
        v = (qp[:, 2:3] - zs).astype(dt)
        lo, hi = dt(c["scan_clip"][0]), dt(c["scan_clip"][1])
        v = np.where(v < lo, lo, np.where(v > hi, hi, v))          # (NaN passes)
        if c["scan_noise"] != 0:
            ctr = counter_hi_lo(episode, ep_len)
            noise = np.stack([c["scan_noise"] * (2.0 * draw(c["seed"], S_SCAN, p & 255, self.genv, ctr) - 1.0) for p in range(px.shape[1])], axis=1)
            v = v + noise.astype(dt)
        return v.astype(dt), np.asarray(frac, dtype=np.float64), over
