"""tests/policy_terrain_reference.py pinned by its properties: ranges of the draws, the level strips, the plane and cell 0 under
the restarted robot, closed forms of the height scan, its invariance to roll and pitch, and the key layout."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_dr_reference as dr_ref  # noqa: E402
from policy_terrain_reference import PolicyTerrainReference, nominal_tables  # noqa: E402

CFG = dict(seed=9, env_offset=3, mass=(0.9, 1.1), friction=(0.4, 1.0), tilt_max=np.deg2rad(8.0), step_height=(0.005, 0.02), step_length=(0.04, 0.12),
           step_prob=0.6, flat_cells=2, num_levels=4, scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7), scan_clip=(-1.0, 1.0))
N = 256


def quat(yaw, pitch=0.0, roll=0.0):
    """wxyz of Rz(yaw) Ry(pitch) Rx(roll), [n, 4]"""
    yaw, pitch, roll = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (yaw, pitch, roll)))
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.stack([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr], axis=-1)


def states(n, seed=0, tilted=True):
    g = np.random.default_rng(seed)
    qpos = np.zeros((n, 7))
    qpos[:, 0:2] = g.uniform(-2, 2, (n, 2))
    qpos[:, 2] = g.uniform(0.2, 0.4, n)
    qpos[:, 3:7] = quat(g.uniform(-np.pi, np.pi, n), g.uniform(-0.5, 0.5, n) * tilted, g.uniform(-0.5, 0.5, n) * tilted)
    return qpos


def fresh_reference(cfg, n=N, seed=0, level=None, dtype=np.float64):
    r = PolicyTerrainReference(n, cfg, dtype)
    qpos = states(n, seed)
    r.reset(np.ones(n), np.arange(n) % 5, qpos, level)
    return r, qpos


def test_draws_lie_in_their_ranges_and_levels_scale_the_height():
    level = np.arange(N) % 6 - 1                       # -1 and 4 are clamped to 0 and 3
    r, qpos = fresh_reference(CFG, level=level)
    ep, tr = r.env_params, r.terrain
    assert (ep[:, 0] >= 0.9).all() and (ep[:, 0] < 1.1).all() and ep[:, 0].std() > 0.03
    assert (ep[:, 1] >= 0.4).all() and (ep[:, 1] < 1.0).all() and ep[:, 1].std() > 0.1
    assert np.allclose(np.linalg.norm(ep[:, 2:5], axis=1), 1.0, atol=1e-15) and (ep[:, 4] > np.cos(CFG["tilt_max"])).all()
    assert (ep[:, 6:] == 0).all()
    assert np.allclose(np.linalg.norm(tr[:, 0:2], axis=1), 1.0, atol=1e-15)
    L = 1.0 / tr[:, 3]
    assert (L >= 0.04 - 1e-15).all() and (L < 0.12).all() and L.std() > 0.015
    lvl = np.clip(level, 0, 3)
    H = tr[:, 4:].max(1)
    some = r.raised.any(1)
    assert some.sum() > N // 2
    assert (H[some] >= 0.005 * (lvl[some] + 1) / 4 - 1e-15).all() and (H[some] < 0.02 * (lvl[some] + 1) / 4).all()
    assert np.array_equal(tr[:, 4:] != 0, r.raised) and (tr[:, 4:][r.raised] == np.broadcast_to(H[:, None], (N, 16))[r.raised]).all()
    assert 0.5 < r.raised[:, 3:14].mean() < 0.7        # step_prob = 0.6 over the strips that may be raised
    # level NULL = the top level
    top, _ = fresh_reference(CFG)
    ref3, _ = fresh_reference(CFG, level=np.full(N, 3))
    assert np.array_equal(top.terrain, ref3.terrain)


@pytest.mark.parametrize("flat", [0, 1, 2, 7])
def test_flat_cells_are_level(flat):
    r, _ = fresh_reference(dict(CFG, flat_cells=flat, step_prob=1.0))
    level = [c for c in range(16) if c <= flat or c >= 16 - flat]
    assert (r.terrain[:, 4 + np.array(level)] == 0).all()
    others = [c for c in range(16) if c not in level]
    assert len(others) == 15 - 2 * flat and (r.terrain[:, 4 + np.array(others, dtype=int)] > 0).all()


def test_plane_and_cell_zero_sit_under_the_restarted_robot():
    r, qpos = fresh_reference(CFG)
    ep, tr = r.env_params, r.terrain
    xb, yb = qpos[:, 0], qpos[:, 1]
    assert np.allclose(ep[:, 2] * xb + ep[:, 3] * yb, ep[:, 5], atol=1e-15)              # the plane passes through (x_b, y_b, 0)
    frac = ((tr[:, 0] * xb + tr[:, 1] * yb) - tr[:, 2]) * tr[:, 3]
    assert np.allclose(frac, 0.5, atol=1e-12)                                            # the middle of cell 0
    # a one-point scan at the base: the height of the base itself
    one = PolicyTerrainReference(N, dict(CFG, scan_x=(0.0, 0.0, 1), scan_y=(0.0, 0.0, 1)))
    one.env_params, one.terrain = ep, tr
    v, f, over = one.scan(qpos)
    assert v.shape == (N, 1) and (over == 0).all() and np.allclose(v[:, 0], qpos[:, 2], atol=1e-14)


def test_only_restarted_rows_change_and_a_degenerate_range_writes_its_value():
    cfg = dict(CFG, mass=(1.05, 1.05), friction=(0.7, 0.7), tilt_max=0.0, step_height=(0.0, 0.0), step_length=(0.1, 0.1))
    r = PolicyTerrainReference(N, cfg)
    before = r.env_params.copy(), r.terrain.copy()
    done = (np.arange(N) % 3 == 0).astype(float)
    fresh = r.reset(done, np.zeros(N, int), states(N))
    assert np.array_equal(fresh, done != 0)
    assert np.array_equal(r.env_params[~fresh], before[0][~fresh]) and np.array_equal(r.terrain[~fresh], before[1][~fresh])
    assert (r.env_params[fresh] == np.array([1.05, 0.7, 0, 0, 1, 0, 0, 0])).all()
    assert (r.terrain[fresh, 4:] == 0).all() and (r.terrain[fresh, 3] == 1.0 / 0.1).all()
    # another episode, another draw; the same episode, the same draw
    a, _ = fresh_reference(CFG)
    b, _ = fresh_reference(CFG)
    assert np.array_equal(a.terrain, b.terrain) and np.array_equal(a.env_params, b.env_params)
    c = PolicyTerrainReference(N, CFG)
    c.reset(np.ones(N), np.arange(N) % 5 + 1, states(N))
    assert (c.env_params[:, 0] != a.env_params[:, 0]).all()


def test_scan_of_a_level_floor_is_the_base_height_at_every_point():
    qpos = states(N)
    for tables in (False, True):
        r = PolicyTerrainReference(N, dict(scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7), scan_clip=(-1.0, 1.0)))
        if tables:                                     # drawn tables of a level floor: flat whatever the strips' geometry
            r.reset(np.ones(N), np.zeros(N, int), qpos)
        v, frac, over = r.scan(qpos, tables=tables)
        assert v.shape == (N, 77) and (v == qpos[:, 2:3]).all() and (over == 0).all()
    # the clip bites, NaN passes
    r = PolicyTerrainReference(N, dict(scan_x=(0.0, 0.1, 2), scan_y=(0.0, 0.0, 1), scan_clip=(0.25, 0.3)))
    q = qpos.copy()
    q[0, 2] = np.nan
    v, _, _ = r.scan(q, tables=False)
    assert np.isnan(v[0]).all() and np.array_equal(v[1:], np.clip(q[1:, 2:3], 0.25, 0.3).repeat(2, 1))


def test_scan_ignores_roll_and_pitch_and_turns_with_yaw():
    cfg = dict(CFG, step_height=(0.0, 0.0))            # a tilted plane: a closed form
    r, _ = fresh_reference(cfg)
    g = np.random.default_rng(4)
    yaw = g.uniform(-np.pi, np.pi, N)
    upright, leaning = states(N, 1), states(N, 1)
    upright[:, 3:7] = quat(yaw)
    leaning[:, 3:7] = quat(yaw, g.uniform(-0.6, 0.6, N), g.uniform(-0.6, 0.6, N))
    a, _, _ = r.scan(upright)
    b, _, _ = r.scan(leaning)
    assert np.abs(a - b).max() < 1e-14
    px, py = r.points()
    assert px.shape == (77,) and px[0] == -0.5 and px[-1] == 0.5 and py[0] == -0.3 and py[6] == 0.3 and py[7] == -0.3 and px[7] == -0.4
    X = upright[:, 0:1] + np.cos(yaw)[:, None] * px - np.sin(yaw)[:, None] * py
    Y = upright[:, 1:2] + np.sin(yaw)[:, None] * px + np.cos(yaw)[:, None] * py
    ep = r.env_params
    want = upright[:, 2:3] - (ep[:, 5:6] - ep[:, 2:3] * X - ep[:, 3:4] * Y) / ep[:, 4:5]
    assert np.abs(a - want).max() < 1e-14 and np.ptp(a, axis=1).min() > 0
    # a degenerate quaternion (base x axis along world z): heading (1, 0)
    q = upright.copy()
    q[:, 3:7] = quat(0.0, np.pi / 2)
    c, _, _ = r.scan(q)
    q[:, 3:7] = quat(0.0)
    d, _, _ = r.scan(q)
    assert np.abs(c - d).max() < 1e-14


def test_scan_sees_the_raised_strips_and_the_noise_is_bounded():
    cfg = dict(CFG, tilt_max=0.0, scan_noise=0.0)
    r, qpos = fresh_reference(cfg)
    v, frac, over = r.scan(qpos)
    assert np.array_equal(over, np.take_along_axis(r.terrain[:, 4:], np.floor(frac).astype(int) & 15, axis=1))
    assert np.abs(v - (qpos[:, 2:3] - over)).max() < 1e-15 and (over > 0).any(1).sum() > N // 2
    noisy = PolicyTerrainReference(N, dict(cfg, scan_noise=0.01))
    noisy.env_params, noisy.terrain = r.env_params, r.terrain
    ep, ln = np.arange(N) % 5 + 1, np.arange(N) % 7
    w, _, _ = noisy.scan(qpos, ep, ln)
    diff = w - v
    assert np.abs(diff).max() <= 0.01 and np.abs(diff).max() > 0.009 and abs(diff.mean()) < 2e-4
    assert len(np.unique(diff)) == diff.size               # every point, env and step its own draw
    w2, _, _ = noisy.scan(qpos, ep, ln + 1)
    assert (w2 != w).all()
    # float32: the same draws, cast once
    low = PolicyTerrainReference(N, CFG, np.float32)
    low.reset(np.ones(N), np.arange(N) % 5, states(N))
    full, _ = fresh_reference(CFG)
    assert low.terrain.dtype == np.float32 and np.array_equal(low.terrain, full.terrain.astype(np.float32))
    assert np.array_equal(low.env_params, full.env_params.astype(np.float32))
    assert low.scan(states(N))[0].dtype == np.float32


def test_streams_12_to_20_collide_with_no_other_key():
    from policy_terrain_reference import S_MASS, S_SCAN
    assert (S_MASS, S_SCAN) == (12, 20)
    for seed in (0, 11, 2 ** 32 - 1):
        keys = {dr_ref.key(seed, s, c) for s in range(1, 21) for c in range(256)}
        assert len(keys) == 20 * 256
        # the restart command draw's keys (any seed below 2^32, + 0, 1, 2) lie below every stream's
        assert min(keys) >= 2 ** 40 > 2 ** 32 + 2
    new = {dr_ref.key(7, s, c) for s in range(12, 21) for c in range(256)}
    old = {dr_ref.key(7, s, c) for s in range(1, 12) for c in range(256)}
    assert not new & old
    # nominal tables: what the sim reads as the nominal model
    ep, tr = nominal_tables(3)
    assert (ep == np.array([1, 1, 0, 0, 1, 0, 0, 0])).all() and (tr[:, 3] == 1).all() and tr.sum() == 3
