"""The numpy restatement of the policy randomisation (tests/policy_dr_reference.py) pinned by its properties: bounds and
means of the draws, distinct keys, the restart draw as resample 0, the push schedule, command zeroing, the yawed quaternion."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_dr_reference as dr  # noqa: E402
from policy_reference import PolicyReference, rot_rows, uniform  # noqa: E402

N_ENV, N_CTR = 4096, 40
ENV = np.repeat(np.arange(N_ENV), N_CTR)
CTR = np.tile(np.arange(1, N_CTR + 1), N_ENV)
NA = 20
ACT_DOF = np.arange(6, 6 + NA)


def make(n, dtype=np.float64, **kw):
    args = dict(cmd_lo=(-0.5, 0.0, -1.0), cmd_hi=(1.0, 0.0, 1.0), seed=11, max_episode_steps=0)
    args.update(kw)
    dr_cfg = args.pop("dr", None)
    return dr.PolicyDRReference(n, ACT_DOF, np.zeros(4, int), (1, 2), np.full(NA, 0.25), np.zeros(NA), dr=dr_cfg, dtype=dtype, **args)


def standing(n):
    qpos, qvel = np.zeros((n, 7 + NA)), np.zeros((n, 6 + NA))
    qpos[:, 2], qpos[:, 3] = 0.33, 1.0
    return qpos, qvel, np.zeros(n, np.int32), np.full((n, 32), -1, np.int32)


def test_noise_lies_within_its_amplitude_and_has_no_mean():
    n = N_ENV * N_CTR
    bound = 4.0 / np.sqrt(3.0 * n)       # 4 sigma of the mean of n uniform(-1, 1) draws (variance 1 / 3)
    for stream in range(1, 12):
        u = dr.draw(7, stream, 3, ENV, CTR)
        assert u.min() >= 0.0 and u.max() < 1.0
        assert abs((2.0 * u - 1.0).mean()) <= bound, (stream, (2.0 * u - 1.0).mean(), bound)
        x = dr.symmetric(7, stream, 3, ENV, CTR, 0.37)
        assert np.abs(x).max() <= 0.37 and np.abs(x).max() > 0.36
    # the obs noise counter: episode * 2^32 + ep_len
    u = dr.draw(7, dr.S_OBS, 0, ENV, dr.counter_hi_lo(np.full(n, 3), CTR))
    assert abs((2.0 * u - 1.0).mean()) <= bound


def test_keys_are_distinct_and_give_different_sequences():
    seed = 123
    keys = {(s, c): dr.key(seed, s, c) for s in range(1, 12) for c in range(256)}
    assert len(set(keys.values())) == len(keys)
    assert not set(keys.values()) & {seed, seed + 1, seed + 2}           # the command draw's keys
    assert min(keys.values()) >= 1 << 40 and dr.key(seed, 1, 0) == seed + (256 << 32) and dr.key(seed, 7, 9) == seed + ((7 * 256 + 9) << 32)
    env, ctr = np.arange(512), np.full(512, 5)
    seqs = {k: dr.draw(seed, k[0], k[1], env, ctr).tobytes() for k in [(s, c) for s in range(1, 12) for c in (0, 1, 19, 64)]}
    seqs["cmd0"], seqs["cmd1"], seqs["cmd2"] = (uniform(seed + i, env, ctr).tobytes() for i in range(3))
    assert len(set(seqs.values())) == len(seqs)
    assert dr.draw(seed, 3, 1, env, ctr).tobytes() != dr.draw(seed + 1, 3, 1, env, ctr).tobytes()


def test_resample_zero_is_the_restart_draw_and_offset_shifts_the_env():
    n = 64
    plain = PolicyReference(n, ACT_DOF, np.zeros(4, int), (1, 2), np.full(NA, 0.25), np.zeros(NA), cmd_lo=(-0.5, 0.0, -1.0),
                            cmd_hi=(1.0, 0.0, 1.0), seed=11)
    rand = make(n, dr=dict(seed=5, command_interval=4, noise_joint_pos=0.01))
    st = standing(n)
    done = np.ones(n)
    for _ in range(3):                                                   # three restarts in a row: episodes 1, 2, 3
        a, b = plain.obs_stage(done, *st), rand.obs_stage(done, *st)
        assert np.array_equal(plain.command, rand.command) and np.array_equal(a[:, 6:9], b[:, 6:9])
        assert np.array_equal(plain.episode, rand.episode) and not rand.resampled.any()
    # the second half of a split batch draws what envs 32 .. 63 of the whole batch draw
    half = make(32, dr=dict(seed=5, command_interval=4, noise_joint_pos=0.01, env_offset=32))
    for _ in range(3):
        o = half.obs_stage(np.ones(32), *standing(32))
    assert np.array_equal(half.command, rand.command[32:]) and np.array_equal(o, b[32:])
    # resamples: at ep_len 4, 8, ... and never at a restart
    cmds = [rand.command.copy()]
    for t in range(1, 10):
        rand.ep_len = np.full(n, t, np.int32)
        rand.obs_stage(np.zeros(n), *st)
        assert rand.resampled.all() == (t % 4 == 0) and rand.resampled.any() == (t % 4 == 0)
        if t % 4:
            assert np.array_equal(rand.command, cmds[-1])
        else:
            assert (rand.command[:, [0, 2]] != cmds[-1][:, [0, 2]]).all() and (rand.command[:, 1] == 0).all()
            assert (rand.command[:, 0] >= -0.5).all() and (rand.command[:, 0] < 1.0).all()
        cmds.append(rand.command.copy())


def test_command_zero_probability_zero_is_never_and_one_is_always():
    n, st = 256, standing(256)
    for prob, frac in ((0.0, 0.0), (1.0, 1.0), (0.25, 0.25)):
        r = make(n, dr=dict(seed=9, command_interval=3, command_zero_prob=prob))
        zeros = events = 0
        r.obs_stage(np.ones(n), *st)
        zeros, events = zeros + int(r.zeroed.sum()), events + n
        assert ((r.command == 0).all(1) == r.zeroed).all()
        for t in range(1, 13):
            r.ep_len = np.full(n, t, np.int32)
            before = r.command.copy()
            r.obs_stage(np.zeros(n), *st)
            if t % 3:
                assert not r.zeroed.any() and np.array_equal(r.command, before)
            else:
                zeros, events = zeros + int(r.zeroed.sum()), events + n
                assert ((r.command == 0).all(1) == r.zeroed).all()
        assert abs(zeros / events - frac) <= (0 if prob in (0.0, 1.0) else 4 * np.sqrt(0.25 * 0.75 / events)), (prob, zeros, events)


def test_push_schedule():
    """after the phase exactly `duration` consecutive active steps out of every `interval`; the force is constant within a
    push, horizontal, lo <= |F| <= hi, and differs between pushes"""
    n, interval, duration, lo, hi, steps = 128, 7, 2, 0.3, 1.0, 50
    env, episode = np.arange(n) + 1000, np.full(n, 3)
    act, frc, ks = [], [], []
    for t in range(steps):
        f, a, k = dr.push_force(21, env, episode, np.full(n, t), interval, duration, lo, hi)
        act.append(a), frc.append(f), ks.append(k)
    act, frc, ks = np.array(act), np.array(frc), np.array(ks)
    phase = np.floor(dr.draw(21, dr.S_PUSH_PHASE, 0, env, episode) * interval).astype(int)
    assert phase.min() == 0 and phase.max() == interval - 1
    for e in range(n):
        want = np.array([t >= phase[e] and (t - phase[e]) % interval < duration for t in range(steps)])
        assert np.array_equal(act[:, e], want)
        starts = [t for t in range(steps) if act[t, e] and (t == 0 or not act[t - 1, e])]
        assert starts == list(range(phase[e], steps, interval))
        for s in starts:
            run = frc[s:s + duration, e]
            assert (run == run[0]).all()
        assert len({frc[s, e].tobytes() for s in starts}) == len(starts)
    mag = np.linalg.norm(frc, axis=2)
    assert (frc[..., 2] == 0).all() and (frc[~act] == 0).all()
    assert (mag[act] >= lo - 1e-15).all() and (mag[act] <= hi + 1e-15).all() and mag[act].max() - mag[act].min() > 0.6
    az = np.arctan2(frc[..., 1], frc[..., 0])[act]
    assert az.min() < -3.0 and az.max() > 3.0                           # all directions
    # another episode, another schedule
    assert not np.array_equal(dr.push_force(21, env, episode + 1, np.full(n, 10), interval, duration, lo, hi)[0], frc[10])
    # the class: ep_len and episode are its own
    r = make(n, dr=dict(seed=21, env_offset=1000, push_interval=interval, push_duration=duration, push_force_lo=lo, push_force_hi=hi))
    r.episode[:], r.ep_len[:] = 3, 10
    f, a = r.perturb()
    assert np.array_equal(f, frc[10]) and np.array_equal(a, act[10])


def test_yawed_quaternion_is_unit_and_keeps_projected_gravity():
    rng = np.random.default_rng(0)
    q = rng.normal(size=(512, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    theta = np.pi * (2 * rng.random(512) - 1)
    out = dr.yaw_quat(q, theta)
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() <= 4 * np.finfo(np.float64).eps
    g0, g1 = -rot_rows(q, np.float64)[:, 2, :], -rot_rows(out, np.float64)[:, 2, :]
    assert np.abs(g0 - g1).max() <= 16 * np.finfo(np.float64).eps
    # and it is the yaw it says: the heading of the body x axis turns by theta
    R0, R1 = rot_rows(q, np.float64), rot_rows(out, np.float64)
    c, s = np.cos(theta), np.sin(theta)
    Rz = np.zeros((512, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1
    assert np.abs(np.einsum("nij,njk->nik", Rz, R0) - R1).max() <= 32 * np.finfo(np.float64).eps
    out32 = dr.yaw_quat(q.astype(np.float32), theta, np.float32)
    assert out32.dtype == np.float32 and np.abs(np.linalg.norm(out32.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps


def test_reset_noise_touches_the_done_envs_only_and_stays_within_its_amplitudes():
    n = 64
    cfg = dict(seed=3, reset_joint_pos=0.1, reset_joint_vel=0.5, reset_base_lin_vel=(0.2, 0.1, 0.0), reset_base_ang_vel=0.5, reset_yaw=np.pi,
               reset_xy=0.3, reset_lift=0.01)
    r = make(n, dr=cfg)
    qpos, qvel, _, _ = standing(n)
    done = (np.arange(n) % 2).astype(float)
    qp, qv = r.reset_noise(done, qpos, qvel)
    f = done != 0
    assert np.array_equal(qp[~f], qpos[~f]) and np.array_equal(qv[~f], qvel[~f])
    assert np.abs(qp[f][:, 7:]).max() <= 0.1 and np.abs(qv[f][:, 6:]).max() <= 0.5 and np.abs(qv[f][:, 3:6]).max() <= 0.5
    assert np.abs(qv[f][:, 0]).max() <= 0.2 and np.abs(qv[f][:, 1]).max() <= 0.1 and (qv[f][:, 2] == 0).all()
    assert np.abs(qp[f][:, :2]).max() <= 0.3 and np.allclose(qp[f][:, 2], 0.34, atol=1e-15)
    assert (qp[f][:, 4:6] == 0).all() and np.abs(np.linalg.norm(qp[f][:, 3:7], axis=1) - 1).max() <= 4e-16
    assert len({row.tobytes() for row in qp[f]}) == int(f.sum())         # every env its own draw
    # the next episode draws anew; float32 casts the same float64 draws
    r.episode += 1
    qp2, _ = r.reset_noise(done, qpos, qvel)
    assert (qp2[f][:, 7:] != qp[f][:, 7:]).all()
    r32 = make(n, np.float32, dr=cfg)
    qp32, qv32 = r32.reset_noise(done, qpos, qvel)
    assert qp32.dtype == np.float32 and np.abs(qp32 - qp).max() <= 1e-6 and np.abs(qv32 - qv).max() <= 1e-6


def test_observation_noise_stays_on_its_columns():
    n = 32
    amp = dict(noise_ang_vel=0.2, noise_gravity=0.05, noise_joint_pos=0.01, noise_joint_vel=1.5)
    clean, noisy = make(n, dr=dict(seed=4)), make(n, dr=dict(seed=4, **amp))
    st = standing(n)
    rng = np.random.default_rng(1)
    st[1][:] = rng.normal(size=st[1].shape)
    a, b = clean.obs_stage(np.ones(n), *st), noisy.obs_stage(np.ones(n), *st)
    diff = b - a
    for cols, amplitude in ((slice(0, 3), 0.2), (slice(3, 6), 0.05), (slice(9, 9 + NA), 0.01), (slice(9 + NA, 9 + 2 * NA), 1.5)):
        assert 0 < np.abs(diff[:, cols]).max() <= amplitude * (1 + 1e-12) and (diff[:, cols] != 0).all()
    exact = np.r_[6:9, 9 + 2 * NA:11 + 3 * NA + 4]
    assert (diff[:, exact] == 0).all()
    # a new step, a new draw; the same step, the same draw
    noisy.ep_len = noisy.ep_len + 1
    c = noisy.obs_stage(np.zeros(n), *st)
    assert (c[:, 0:3] != b[:, 0:3]).all()
    assert np.array_equal(noisy.obs_stage(np.zeros(n), *st), c)
