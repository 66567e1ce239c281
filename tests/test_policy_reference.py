"""tests/policy_reference.py, the numpy restatement of the policy environment's kernels, pinned by closed forms and
invariances on a toy robot (4 actuators, 5 bodies with one geom each, soles on bodies 3 and 4) - no GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_reference import HIST, NPRIV, NT, TERMS, PolicyReference, plan_hash, uniform  # noqa: E402

NA, NQ, NV = 4, 11, 10
ACT_DOF = [6, 8, 7, 9]            # (not the identity: the actuator order is not the dof order)
GEOM_BODY = [0, 1, 2, 3, 4]
FEET = (3, 4)
T = TERMS.index


def ref(n=3, **kw):
    kw.setdefault("scale", np.full(NA, 0.25))
    kw.setdefault("default", np.array([0.1, -0.2, 0.3, 0.0]))
    return PolicyReference(n, ACT_DOF, GEOM_BODY, FEET, kw.pop("scale"), kw.pop("default"), **kw)


def standing(n, z=0.33):
    qpos, qvel = np.zeros((n, NQ)), np.zeros((n, NV))
    qpos[:, 2], qpos[:, 3] = z, 1.0
    return qpos, qvel


def contacts(n, geoms=((3, 4),)):
    """ncon, con_pairs with floor rows on the given geoms (one tuple per env, repeated to n)"""
    ncon, cp = np.zeros(n, np.int32), np.full((n, 32), -1, np.int32)
    for e in range(n):
        gs = geoms[e % len(geoms)]
        ncon[e] = len(gs)
        for i, g in enumerate(gs):
            cp[e, i] = (g << 16) | (7 + i)
    return ncon, cp


INFO = lambda n: np.zeros((n, 4), np.int32)


def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def test_upright_at_rest_has_gravity_down_and_no_penalties():
    r = ref(h_target=0.33, weights={k: 1.0 for k in TERMS})
    qpos, qvel = standing(3)
    qpos[:, 7:] = np.asarray(r.default)[np.argsort(ACT_DOF)]          # joints at the default pose
    qpos[:, 7 + np.asarray(ACT_DOF) - 6] = r.default
    ncon, cp = contacts(3)
    rew, done = r.reward_stage(qpos, qvel, ncon, cp, INFO(3))
    o = r.obs_stage(done, qpos, qvel, ncon, cp)
    assert np.array_equal(o[:, 3:6], np.tile([0.0, 0.0, -1.0], (3, 1)))
    assert np.array_equal(o[:, 0:3], np.zeros((3, 3))) and np.array_equal(o[:, 9:9 + 2 * NA], np.zeros((3, 2 * NA)))
    assert np.array_equal(o[:, 9 + 3 * NA:11 + 3 * NA], np.ones((3, 2)))          # both soles on the floor
    assert np.array_equal(o[:, r.nobs:], np.tile([0.0, 0.0, 0.0, 0.33], (3, 1))) and o.shape[1] == 11 + 3 * NA + NPRIV
    for k in ("lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "action_rate", "joint_vel", "feet_air_time", "termination"):
        assert np.array_equal(r.terms[:, T(k)], np.zeros(3)), k
    assert np.array_equal(r.terms[:, T("alive")], np.ones(3)) and np.array_equal(r.terms[:, T("track_lin_vel")], np.ones(3))
    assert np.array_equal(rew, np.full(3, 3.0)) and not done.any() and not r.timeout.any()   # alive + the two tracking terms


def test_yaw_rotation_changes_neither_obs_nor_terms():
    rng = np.random.default_rng(0)
    n = 6
    qpos, qvel = standing(n)
    q = rng.normal(size=(n, 4)) * 0.2 + np.array([1.0, 0, 0, 0])
    qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    qpos[:, 7:], qvel[:] = rng.normal(size=(n, NA)) * 0.3, rng.normal(size=(n, NV))
    ncon, cp = contacts(n, ((3,), (4,), ()))
    out = []
    for yaw in (0.0, 0.7, -2.9):
        r = ref(n, weights={k: 0.5 for k in TERMS}, cmd_lo=(0.4, -0.1, 0.3), cmd_hi=(0.4, -0.1, 0.3))
        r.air[:] = 0.3
        qp, qv = qpos.copy(), qvel.copy()
        c, s = np.cos(yaw), np.sin(yaw)
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        yq = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
        for e in range(n):
            qp[e, 3:7] = quat_mul(yq, qpos[e, 3:7])      # world-frame yaw on top of the orientation
            qv[e, 0:3] = Rz @ qvel[e, 0:3]               # the world-frame linear velocity turns with it; the rest is body-frame
        rew, done = r.reward_stage(qp, qv, ncon, cp, INFO(n))
        tilt_done = r.terms[:, T("termination")].copy()
        out.append((r.terms.copy(), rew.copy(), r.obs_stage(np.zeros(n), qp, qv, ncon, cp).copy(), tilt_done))
    for terms, rew, o, _ in out[1:]:
        assert np.abs(terms - out[0][0]).max() < 1e-14 and np.abs(rew - out[0][1]).max() < 1e-14 and np.abs(o - out[0][2]).max() < 1e-14


def test_tracking_terms_are_one_at_the_commanded_velocity():
    n = 4
    r = ref(n, cmd_lo=(0.5, -0.2, 0.8), cmd_hi=(0.5, -0.2, 0.8), sigma=0.25)
    qpos, qvel = standing(n)
    yaw = np.array([0.0, 0.5, 1.5, -2.0])
    qpos[:, 3], qpos[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    qvel[:, 0] = np.cos(yaw) * 0.5 + np.sin(yaw) * 0.2          # world velocity of the body-frame (0.5, -0.2, 0)
    qvel[:, 1] = np.sin(yaw) * 0.5 - np.cos(yaw) * 0.2
    qvel[:, 5] = 0.8
    ncon, cp = contacts(n)
    r.reward_stage(qpos, qvel, ncon, cp, INFO(n))
    assert np.abs(r.terms[:, T("track_lin_vel")] - 1).max() < 1e-14 and np.array_equal(r.terms[:, T("track_ang_vel")], np.ones(n))
    # and fall off as the Gaussian says: 0.25 m/s off in x -> exp(-1)
    qvel[:, 0] += np.cos(yaw) * 0.25
    qvel[:, 1] += np.sin(yaw) * 0.25
    r.reward_stage(qpos, qvel, ncon, cp, INFO(n))
    assert np.abs(r.terms[:, T("track_lin_vel")] - np.exp(-1.0)).max() < 1e-14


@pytest.mark.parametrize("d", [0, 1, 3, 7])
def test_delay_shifts_the_ctrl_sequence(d):
    rng = np.random.default_rng(1)
    n, steps = 2, 20
    actions = rng.uniform(-1, 1, size=(steps, n, NA))
    r0, rd = ref(n), ref(n)
    rd.delay[:] = d
    qpos, qvel = standing(n)
    ncon, cp = contacts(n)
    seq0, seqd = [], []
    for t in range(steps):
        for r, seq in ((r0, seq0), (rd, seqd)):
            seq.append(r.act(actions[t]).copy())
            r.reward_stage(qpos, qvel, ncon, cp, INFO(n))       # (advances ep_len)
            r.obs_stage(r.done, qpos, qvel, ncon, cp)
    for t in range(steps):
        want = seq0[t - d] if t >= d else np.tile(r0.default, (n, 1))     # nothing in the ring yet: the default pose
        assert np.array_equal(seqd[t], want), t


def test_alpha_one_returns_the_target_bit_for_bit_and_the_filter_converges():
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, size=(3, NA))
    r = ref(3, alpha=1.0)
    r.ctrl[:] = rng.normal(size=(3, NA))                       # whatever ctrl held before
    assert np.array_equal(r.act(a), r.default + r.scale * a)
    f = ref(3, alpha=0.5)
    c1 = f.act(a).copy()
    assert np.allclose(c1, 0.5 * (f.default + f.scale * a), rtol=0, atol=1e-15)       # from ctrl = 0
    for _ in range(60):
        f.ep_len += 1
        c = f.act(a)
    assert np.abs(c - (f.default + f.scale * a)).max() < 1e-15
    # clipping, and NaN passing through
    k = ref(1, clip=0.5)
    got = k.act(np.array([[2.0, -2.0, 0.25, np.nan]]))
    assert np.array_equal(k.last[0, :3], [0.5, -0.5, 0.25]) and np.isnan(k.last[0, 3]) and np.isnan(got[0, 3])


def test_timeout_and_termination_are_exclusive():
    n = 5
    r = ref(n, max_episode_steps=3, weights=dict(termination=-10.0, alive=1.0))
    qpos, qvel = standing(n)
    qpos[1, 2] = 0.1                                            # below done_height
    qpos[2, 3:7] = [np.cos(0.5), np.sin(0.5), 0, 0]            # rolled by 1 rad: up = cos(1) < cos(45 deg)
    ncon, cp = contacts(n, ((3, 4), (3, 4), (3, 4), (0, 3), (3, 4)))   # env 3: the torso (mask bit 0) on the floor
    info = INFO(n)
    for step in range(3):
        if step == 2:
            info[4, 3] = 4                                      # env 4: its sim step was skipped on the last step
        rew, done = r.reward_stage(qpos, qvel, ncon, cp, info)
        term, to = r.terms[:, T("termination")] != 0, r.timeout != 0
        assert not (term & to).any() and np.array_equal(done != 0, term | to)
        assert np.array_equal(term, [False, True, True, True, step == 2]) and np.array_equal(to, [step == 2, False, False, False, False])
        assert np.array_equal(rew, np.where(term, -9.0, 1.0))
        r.obs_stage(done, qpos, qvel, ncon, cp)
    assert r.ep_len.tolist() == [0, 0, 0, 0, 0] and r.episode.tolist() == [1, 3, 3, 3, 1]
    # a robot<->robot row (bit 0x8000) on the torso's geom does not terminate, a non-finite state does
    r = ref(2)
    qpos, qvel = standing(2)
    qvel[1, 7] = np.inf
    ncon, cp = contacts(2)
    cp[0, 2], ncon[0] = (3 << 16) | 0x8000 | 0, 3
    r.reward_stage(qpos, qvel, ncon, cp, INFO(2))
    assert r.terms[:, T("termination")].tolist() == [0.0, 1.0]


def test_air_time_over_a_scripted_contact_sequence():
    r = ref(1, decimation=10, sim_dt=0.002, t_air=0.05, cmd_lo=(0.5, 0, 0), cmd_hi=(0.5, 0, 0), deadband=0.1)
    qpos, qvel = standing(1)
    # left sole: down, up for 4 steps, down (first contact after 0.08 s), down; the right sole stays down
    script = [(3, 4), (4,), (4,), (4,), (4,), (3, 4), (3, 4)]
    want_air = [0.0, 0.02, 0.04, 0.06, 0.08, 0.0, 0.0]
    want_term = [0, 0, 0, 0, 0, 0.08 - 0.05, 0]
    for g, a, t in zip(script, want_air, want_term):
        ncon, cp = contacts(1, (g,))
        r.reward_stage(qpos, qvel, ncon, cp, INFO(1))
        assert abs(r.terms[0, T("feet_air_time")] - t) < 1e-15 and abs(r.air[0, 0] - a) < 1e-15 and r.air[0, 1] == 0, (g, r.air, r.terms[0])
    # below the deadband the term is zero, the bookkeeping the same
    s = ref(1, t_air=0.05)
    for g, a in zip(script, want_air):
        ncon, cp = contacts(1, (g,))
        s.reward_stage(qpos, qvel, ncon, cp, INFO(1))
        assert s.terms[0, T("feet_air_time")] == 0 and abs(s.air[0, 0] - a) < 1e-15
    # a reset zeroes it and reports both feet down whatever the stale list says
    ncon, cp = contacts(1, ((),))
    s.air[:] = 0.3
    o = s.obs_stage(np.ones(1), qpos, qvel, ncon, cp)
    assert np.array_equal(s.air, np.zeros((1, 2))) and o[0, 9 + 3 * NA:11 + 3 * NA].tolist() == [1.0, 1.0]
    assert s.obs_stage(np.zeros(1), qpos, qvel, ncon, cp)[0, 9 + 3 * NA:11 + 3 * NA].tolist() == [0.0, 0.0]


def test_redrawn_commands_lie_in_range_and_are_reproducible():
    # the hash: SplitMix64's finaliser of the mixed key, a fixed value and full-width arithmetic
    assert int(plan_hash(0, 0, 0)[0]) == 0xE220A8397B1DCDAF      # splitmix64(0)'s first output
    n = 512
    lo, hi = (-0.5, 0.2, -1.0), (1.0, 0.2, 1.0)
    a, b = ref(n, seed=7, cmd_lo=lo, cmd_hi=hi), ref(n, seed=7, cmd_lo=lo, cmd_hi=hi)
    qpos, qvel = standing(n)
    ncon, cp = contacts(n)
    seen = []
    for ep in range(4):
        for r in (a, b):
            r.obs_stage(np.ones(n), qpos, qvel, ncon, cp)
        assert np.array_equal(a.command, b.command) and a.episode.tolist() == [ep + 1] * n
        assert (a.command[:, 0] >= lo[0]).all() and (a.command[:, 0] < hi[0]).all() and (a.command[:, 2] >= lo[2]).all() and (a.command[:, 2] < hi[2]).all()
        assert np.array_equal(a.command[:, 1], np.full(n, 0.2))             # lo == hi: never redrawn
        assert np.array_equal(a.obs[:, 6:9], a.command)
        seen.append(a.command.copy())
    # envs, episodes and components all draw differently, another seed too; envs that are not done keep theirs
    assert len(np.unique(np.concatenate(seen)[:, 0])) == 4 * n and not np.array_equal(seen[0][:, 0], seen[0][:, 2])
    assert abs(np.concatenate(seen)[:, 0].mean() - 0.25) < 0.05
    c = ref(n, seed=8, cmd_lo=lo, cmd_hi=hi)
    c.obs_stage(np.ones(n), qpos, qvel, ncon, cp)
    assert not np.array_equal(c.command, seen[0])
    keep = a.command.copy()
    part = np.zeros(n)
    part[::2] = 1
    a.obs_stage(part, qpos, qvel, ncon, cp)
    assert np.array_equal(a.command[1::2], keep[1::2]) and not np.array_equal(a.command[::2, 0], keep[::2, 0])
    assert np.array_equal(uniform(7, np.arange(n), a.episode)[::2] * 1.5 - 0.5, a.command[::2, 0])


def test_float32_arithmetic_stays_float32():
    r = ref(2, dtype=np.float32, weights={k: 1.0 for k in TERMS}, alpha=0.5, cmd_lo=(0, 0, 0), cmd_hi=(1, 0, 0))
    qpos, qvel = standing(2)
    ncon, cp = contacts(2)
    assert r.act(np.full((2, NA), 0.3)).dtype == np.float32
    rew, done = r.reward_stage(qpos, qvel, ncon, cp, INFO(2), act_force=np.ones((2, NA)))
    o = r.obs_stage(np.ones(2), qpos, qvel, ncon, cp)
    assert rew.dtype == done.dtype == o.dtype == r.terms.dtype == r.air.dtype == r.ctrl.dtype == r.command.dtype == np.float32
    assert NT == 12 and HIST == 8
