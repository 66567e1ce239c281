"""Site sensors of the sim stage (tsidb_set_sensors / WalkController.enable_sensors; what a caller of mj_step reads as
mj_data.sensordata: framepos, framequat, framelinvel, frameangvel, velocimeter, gyro, accelerometer): against the numpy
restatement of tests/sensor_reference.py (pinned on the CPU by tests/test_sensor_reference.py) from the state a step starts
from and the device's own qacc of that step, physics checks that pin the timing and the frames, bit-identity of the state
with and without sensors, every step path, and the contract of the C entry point."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sensor_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SIM_STATE = ("q", "v", "tau", "dv", "f", "status", "rows", "qpos", "qvel", "qacc_warmstart", "ncon", "con_pairs", "info")
READOUTS = ("con_force", "con_frame", "con_pos", "con_dist", "actuator_force", "foot_force", "foot_cop")
# float64: the project's parity contract: the state tolerance on pose and velocity entries, the dv
# tolerance on the accelerometer, plus 1e-12 of the reference entry's magnitude (touch-down accelerations reach 1e3 m/s^2)
F64_STATE, F64_ACC, F64_REL = 1e-9, 1e-7, 1e-12
# float32: section 5's rtol 1e-3 / atol 1e-4 on pose and velocity entries; the accelerometer at the tolerance DESIGN.md
# section 2 amends qvel to because of the stiff contact rows, 5e-5, over dt (qvel carries dt x qacc): 2.5e-2 m/s^2 at 2 ms
F32_ATOL, F32_RTOL, F32_QVEL = 1e-4, 1e-3, 5e-5


def make(n, dtype="f64", v0=False, **over):
    from tsid_control_amd import RobotConfig, WalkController, op3_v0_conf
    conf = op3_v0_conf() if v0 else RobotConfig()
    conf.dtype = dtype
    for k, v in over.items():
        setattr(conf, k, v)
    return WalkController(conf, num_envs=n, device="cuda:0")


def walker(n, dtype="f64", closed=False, **over):
    """the walking workload (tools/sim_readouts.py): open loop, or closed loop with touch-down feedback"""
    from tsid_control_amd import RobotConfig, WalkController
    from tsid_control_amd.walk_planner import WalkSchedule, op3_closed_loop_walking_conf, op3_walking_conf, op3_walking_posture
    conf = op3_closed_loop_walking_conf(RobotConfig()) if closed else op3_walking_conf(RobotConfig())
    conf.dtype = dtype
    for k, v in over.items():
        setattr(conf, k, v)
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    wc.posture_ref += torch.as_tensor(op3_walking_posture(), device=wc.device).to(wc.dtype)
    lf, rf = wc.frames[0, 0, 9:11].cpu().numpy(), wc.frames[0, 1, 9:11].cpu().numpy()
    sched = WalkSchedule.from_demo_paths(n, conf, wc.device, wc.dtype, seed=1, q0_feet=(lf, rf),
                                         com0=wc.com_ref[0, :3].double().cpu().numpy(), foot_press=0.0, t_start=0.5)
    if closed:
        sched.enable_touchdown_feedback(0.6)
    return wc, sched


def perturb(wc, seed, spread=0.02):
    g = torch.Generator().manual_seed(seed)
    wc.qpos[:, 7:] += ((torch.rand(wc.num_envs, wc.NQ - 7, generator=g, dtype=torch.float64) - 0.5) * spread).to(wc.device, wc.dtype)


def same(a, b, keys=SIM_STATE):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y), (k, (x != y).nonzero()[:6].tolist())


def foot_bodies(blob):
    fp, s2t = blob["pin_frame_parent"][:2], list(blob["mj_sim2tsid"])
    return [1 + s2t.index(int(fp[f]) - 1) for f in range(2)]


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def sites_for(wc):
    """torso, both soles and an arm body, offsets of centimetres, generic orientations (one a half turn about an oblique
    axis, w = 0: the case the quaternion conversion has to survive)"""
    lf, rf = foot_bodies(wc.model)
    arm = wc.NB - 5
    return [(0, [0.01, -0.02, 0.05], unit([0.8, 0.1, -0.5, 0.3])),
            (lf, [0.02, 0.01, -0.015], unit([0.3, -0.7, 0.2, 0.6])),
            (rf, [-0.01, 0.03, -0.02], unit([0.0, 0.6, -0.3, 0.74])),
            (arm, [0.0, 0.04, 0.03], unit([-0.5, 0.5, 0.4, 0.58]))]


def reference(wc, fk, qpos, qvel, qacc, sites, envs):
    return np.stack([sr.sensors(wc.model, qpos[e], qvel[e], qacc[e], sites, fk) for e in envs])


def errors(got, want, f32=False, dt=0.002):
    """worst absolute errors (pose and velocity entries, quaternions up to sign; accelerometer) and the worst ratio of an
    error to its gate"""
    got, want = np.asarray(got, dtype=np.float64), want.copy()
    want[..., 3:7] = sr.align_quat(got[..., 3:7], want[..., 3:7])
    d = np.abs(got[..., :22] - want)
    atol = np.full(22, F32_ATOL if f32 else F64_STATE)
    atol[19:22] = F32_QVEL / dt if f32 else F64_ACC
    gate = atol + (F32_RTOL if f32 else F64_REL) * np.abs(want)
    return dict(pose_vel=float(d[..., :19].max()), acc=float(d[..., 19:22].max()), ratio=float((d / gate).max()),
                acc_max=float(np.abs(want[..., 19:22]).max()), spare=float(np.abs(got[..., 22:]).max()))


def teacher_forced(wc, fk, sites, steps, envs, advance, f32=False):
    """single steps, each compared with the reference at the state the step started from and the device's own qacc of
    that step (qacc_warmstart: the step writes its qacc as the next warm start; held to the oracle by the parity tests)"""
    worst = dict(pose_vel=0.0, acc=0.0, ratio=0.0, acc_max=0.0, spare=0.0)
    for i in range(steps):
        qpos, qvel = wc.qpos.double().cpu().numpy().copy(), wc.qvel.double().cpu().numpy().copy()
        advance(i)
        torch.cuda.synchronize()
        assert int((wc.info[:, 3] & 4).sum()) == 0
        qacc = wc.qacc_warmstart.double().cpu().numpy()
        e = errors(wc.sensordata.cpu().numpy()[envs], reference(wc, fk, qpos, qvel, qacc, sites, envs), f32, wc.conf.dt)
        worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


def scenarios(dtype, v0, with_walking):
    """(name, worst errors) of the teacher-forced cases: perturbed standing pressed into the floor; lifted generic poses
    with base and joint velocities; a touch-down - for the v1 robot a stretch of closed-loop walking through the first
    step's touch-down, for the v0 robot (which has no walking workload in this project) closed-loop standing dropped from
    5 mm above the floor"""
    f32 = dtype == "f32"
    out = []
    n = 64
    wc = make(n, dtype, v0=v0)
    fk, sites = sr.FK(wc.model), sites_for(wc)
    perturb(wc, 7, spread=0.1)
    wc.qpos[:, 2] -= 0.002
    wc.enable_sensors(sites)
    w = teacher_forced(wc, fk, sites, 4, range(n), lambda i: wc.sim_step(teleport=False), f32)
    assert int(wc.ncon.min()) > 0
    out.append(("standing", w))

    wc = make(n, dtype, v0=v0, self_collision=False)
    g = torch.Generator().manual_seed(21)
    wc.qpos[:, 2] += 1.0
    wc.qpos[:, 7:] += ((torch.rand(n, wc.NQ - 7, generator=g, dtype=torch.float64) - 0.5) * 0.6).to(wc.device, wc.dtype)
    quat = torch.randn(n, 4, generator=g, dtype=torch.float64)
    wc.qpos[:, 3:7] = (quat / quat.norm(dim=1, keepdim=True)).to(wc.device, wc.dtype)
    wc.qvel[:] = (torch.randn(n, wc.NV, generator=g, dtype=torch.float64) * 0.8).to(wc.device, wc.dtype)
    wc.enable_sensors(sites)
    w = teacher_forced(wc, fk, sites, 3, range(n), lambda i: wc.sim_step(teleport=False), f32)
    assert int(wc.ncon.max()) == 0
    out.append(("lifted", w))

    if with_walking and not v0:
        wc, sched = walker(n, dtype, closed=True)
        wc.enable_sim_readouts()
        wc.enable_sensors(sites)

        def advance(i):
            sched.apply(wc, wc.t)
            wc.step()
        for i in range(380):                          # the start phase and most of the first swing
            advance(i)
        touched = 0
        envs = range(0, n, 8)
        loaded = wc.foot_force[:, :, 2] > 0

        def advance_and_count(i):
            nonlocal touched, loaded
            advance(i)
            now = wc.foot_force[:, :, 2] > 0
            touched += int((now & ~loaded)[list(envs)].sum())
            loaded = now
        w = teacher_forced(wc, fk, sites, 150, envs, advance_and_count, f32)
        assert touched > 0, "no sole touched down in the compared stretch"
        assert int((wc.done != 0).sum()) == 0
        out.append(("walking", w))
    elif with_walking:
        wc = make(n, dtype, v0=True, closed_loop=True, reference_quirks=False)
        perturb(wc, 5)
        wc.qpos[:, 2] += 0.005
        wc.enable_sensors(sites)
        w = teacher_forced(wc, fk, sites, 60, range(0, n, 4), lambda i: wc.step(), f32)
        assert int(wc.ncon.min()) > 0 and w["acc_max"] > 15.0, w    # (it did land: more than gravity's 9.81)
        out.append(("drop", w))
    return out


# ---------------------------------------------------------------------------- 1. against the numpy reference, float64
@pytest.mark.parametrize("v0", [False, True])
def test_sensors_match_the_numpy_reference_f64(v0):
    """Measured worst cases (MI355X) are recorded in DESIGN.md section 4 "Site sensors"."""
    for name, w in scenarios("f64", v0, with_walking=True):
        print(f"f64 {'v0' if v0 else 'v1'} {name}: pose / velocity {w['pose_vel']:.2e}, accelerometer {w['acc']:.2e} "
              f"(largest reference {w['acc_max']:.3g} m/s^2), worst error / gate {w['ratio']:.2e}")
        assert w["ratio"] <= 1.0 and w["spare"] == 0.0, (name, w)


# ---------------------------------------------------------------------------- 2. free fall pins the timing
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_free_fall_pins_the_timing(dtype):
    """No constraint rows, no joint forces (joint angles exactly 0 = the servo targets), at rest 1 m up: after step k the
    torso site shows the state BEFORE step k under semi-implicit Euler - velocity -(k - 1) g dt, height z0 - g dt^2 (k - 1) k
    / 2 (post-step semantics would be off by one g dt = 2e-2 m/s) - and every accelerometer and gyro reads zero.
    Gates: f64 the state tolerance 1e-9; f32 rtol 1e-3 / atol 1e-4, the accelerometer 1e-3 g (its two terms, the solved
    acceleration and gravity, cancel: float32's relative tolerance on each)."""
    n = 64
    wc = make(n, dtype, sim_frictionloss_scale=0.0, self_collision=False)
    wc.qpos[:, 2] += 1.0
    wc.qpos[:, 7:] = 0.0
    z0 = wc.qpos[:, 2].double().cpu().numpy().copy()
    wc.enable_sensors(sites_for(wc) + ["imu"])
    g, dt = 9.81, wc.conf.dt
    f32 = dtype == "f32"
    worst = dict(v=0.0, z=0.0, acc=0.0, gyro=0.0)
    for k in range(1, 7):
        wc.sim_step(teleport=False)
        torch.cuda.synchronize()
        assert int(wc.ncon.max()) == 0 and int((wc.info[:, 3] & 4).sum()) == 0
        s = wc.sensordata.double().cpu().numpy()
        vz, z = -(k - 1) * g * dt, z0 - g * dt * dt * (k - 1) * k / 2
        ev, ez = np.abs(s[:, 4, 9] - vz).max(), np.abs(s[:, 4, 2] - z).max()
        worst = dict(v=max(worst["v"], ev), z=max(worst["z"], ez), acc=max(worst["acc"], np.abs(s[:, :, 19:22]).max()),
                     gyro=max(worst["gyro"], np.abs(s[:, :, 16:19]).max()))
        tol_v, tol_z = (F32_ATOL + F32_RTOL * abs(vz), F32_ATOL + F32_RTOL * np.abs(z).max()) if f32 else (F64_STATE, F64_STATE)
        assert ev <= tol_v and ez <= tol_z, (k, ev, ez)
        assert np.abs(s[:, 4, 7:9]).max() <= (F32_ATOL if f32 else F64_STATE)
    print(f"{dtype} free fall: velocity {worst['v']:.2e}, height {worst['z']:.2e}, accelerometer {worst['acc']:.2e}, gyro {worst['gyro']:.2e}")
    assert worst["acc"] <= (F32_RTOL * g if f32 else 1e-9), worst
    assert worst["gyro"] <= (F32_ATOL if f32 else 1e-9), worst


# ---------------------------------------------------------------------------- 3. uniform acceleration field
def test_uniform_field_reads_on_every_accelerometer():
    """test_uniform_field_shifts_only_the_base_acceleration's wrenches, F_b = m_b a on every body in free flight: every
    site on every body reads accelerometer(e) - accelerometer(0) = R_site^T a_e against the unpushed env 0"""
    n = 4
    a = torch.tensor([[0.0, 0.0, 0.0], [15.0, -10.0, 25.0], [-20.0, 5.0, 0.0], [2.5, 30.0, -10.0]], dtype=torch.float64)
    worst = 0.0
    for lo in (0, None):                                       # two site tables: bodies 0 .. 15, then the last 16
        wc = make(n, sim_frictionloss_scale=0.0, self_collision=False)
        bodies = list(range(16)) if lo == 0 else list(range(wc.NB - 16, wc.NB))
        rng = np.random.default_rng(2)
        sites = [(b, rng.normal(size=3) * 0.03, unit(rng.normal(size=4))) for b in bodies]
        wc.set_env_params(mass_scale=torch.full((n,), 1.1, dtype=torch.float64))
        wc.qpos[:, 2] += 1.0
        m = wc.body_masses()
        w = torch.zeros(n, wc.NB, 6, dtype=wc.dtype, device=wc.device)
        w[:, :, :3] = m[:, :, None] * a.to(wc.device)[:, None, :]
        wc.set_xfrc(w)
        wc.enable_sensors(sites)
        qpos = wc.qpos[0].cpu().numpy().copy()
        wc.sim_step(teleport=False)
        torch.cuda.synchronize()
        assert int(wc.ncon.max()) == 0 and int((wc.info[:, 3] & 4).sum()) == 0
        _, Rs = sr.FK(wc.model).site_pose(qpos, sites)
        acc = wc.accelerometer.cpu().numpy()
        for e in range(1, n):
            want = np.einsum("sji,j->si", Rs, a[e].numpy())
            worst = max(worst, np.abs(acc[e] - acc[0] - want).max())
    print(f"uniform field: {worst:.2e}")
    assert worst <= 1e-9, worst


# ---------------------------------------------------------------------------- 4. standing
def test_standing_accelerometer_reads_gravity():
    """1000 closed-loop standing steps (2 s): the torso accelerometer is within the settled residual of R^T (0, 0, g):
    |acc - R^T g| <= |J qacc| of the same step (the reference's site Jacobian times the device's qacc) + 1e-9"""
    n = 64
    wc = make(n, closed_loop=True)
    perturb(wc, 5)
    wc.enable_sensors(["imu"])
    for _ in range(999):
        wc.step()
    qpos = wc.qpos.cpu().numpy().copy()
    wc.step()
    torch.cuda.synchronize()
    assert int((wc.done != 0).sum()) == 0
    qacc, acc, quat = wc.qacc_warmstart.cpu().numpy(), wc.accelerometer.cpu().numpy()[:, 0], wc.framequat.cpu().numpy()[:, 0]
    fk, site = sr.FK(wc.model), [(0, np.zeros(3), np.array([1.0, 0, 0, 0]))]
    worst = resid = 0.0
    for e in range(n):
        R = sr.quat_to_mat(quat[e])
        d = np.linalg.norm(acc[e] - R.T @ np.array([0, 0, 9.81]))
        jq = np.linalg.norm(sr.site_jacobian_acc(wc.model, qpos[e], qacc[e], site, fk)[0])
        worst, resid = max(worst, d - jq), max(resid, jq)
    print(f"standing: largest |J qacc| {resid:.2e} m/s^2, largest |acc - R^T g| - |J qacc| {worst:.2e}")
    assert worst <= 1e-9, (worst, resid)


# ---------------------------------------------------------------------------- 5. bit-identity
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sensors_do_not_perturb_the_step(dtype):
    """300 walking steps (open loop: single steps, then the pipelined step's batched launches) with sensors registered
    against a controller without: state, contact lists and info bit-identical, and the readouts where they are on; then
    enable -> disable returns to the plain kernels"""
    for ro in (False, True):
        (a, sa), (b, sb) = walker(64, dtype, pipeline_sim_batch=4), walker(64, dtype, pipeline_sim_batch=4)
        if ro:
            a.enable_sim_readouts(); b.enable_sim_readouts()
        b.enable_sensors(sites_for(b))
        for i in range(300):
            if i < 200:
                sa.apply(a, a.t); sb.apply(b, b.t)
                a.step(); b.step()
            else:
                a.step_pipelined(walk=(sa, a.t)); b.step_pipelined(walk=(sb, b.t))
        a.sync_sim(); b.sync_sim()
        same(a, b)
        if ro:
            same(a, b, READOUTS)
        assert int(b.ncon.sum()) > 0 and float(b.gyro.abs().sum()) > 0
        buf = b.sensordata
        kept = buf.clone()
        b.disable_sensors()
        assert b.sensordata is None and b.gyro is None
        for i in range(20):
            sa.apply(a, a.t); sb.apply(b, b.t)
            a.step(); b.step()
        same(a, b)
        torch.cuda.synchronize()
        assert torch.equal(buf, kept)                         # (the buffer is no longer written)


def test_sensors_keep_the_f32_three_wave_build_bit_identical():
    """float32 at >= 3072 envs: the three-waves-per-SIMD build has no sensor instantiation; the default build that runs
    instead is bit-identical to it"""
    a, b = make(3072, "f32"), make(3072, "f32")
    for wc in (a, b):
        perturb(wc, 4)
    b.enable_sensors(["imu", "lf_imu", "rf_imu"])
    for _ in range(10):
        a.step(); b.step()
    same(a, b)
    assert float(b.accelerometer.abs().sum()) > 0


# ---------------------------------------------------------------------------- 6. every step path
def test_every_step_path_writes_the_same_rows():
    """eager step(), step_pipelined() + sync_sim() with launches of 1 and of 8 sim steps (tsidb_sim_batch leaves the last
    step's rows), one and two wavefronts per env, and a capture_steps() graph: the same rows, bit for bit"""
    def w(**over):
        wc, _ = walker(64, **over)
        perturb(wc, 13)
        wc.apply_push([0.0, 2.0, 0.5], body=14, env_ids=range(0, 64, 3))
        wc.enable_sensors(sites_for(wc))
        return wc
    eager, eager1, pipe, batched, graph = (w(pipeline_sim_batch=1), w(pipeline_sim_batch=1, sim_waves=1), w(pipeline_sim_batch=1),
                                           w(pipeline_sim_batch=8), w(pipeline_sim_batch=1))
    batched1 = w(pipeline_sim_batch=8, sim_waves=1)
    for _ in range(16):
        eager.step(); eager1.step(); graph.step()
        pipe.step_pipelined(); batched.step_pipelined(); batched1.step_pipelined()
    for wc in (pipe, batched, batched1):
        wc.sync_sim()
    for other in (eager1, pipe, batched, batched1, graph):
        same(eager, other)
        assert torch.equal(eager.sensordata, other.sensordata), (eager.sensordata != other.sensordata).nonzero()[:6].tolist()
    g = graph.capture_steps(8)
    for _ in range(8):
        eager.step()
    g.replay()
    graph.sync_sim()
    torch.cuda.synchronize()
    same(eager, graph)
    assert torch.equal(eager.sensordata, graph.sensordata)
    assert float(eager.accelerometer.abs().min(dim=2).values.max()) > 0 and int(eager.ncon.sum()) > 0


# ---------------------------------------------------------------------------- 7. contract
def test_skipped_step_reset_and_substeps():
    a, b = make(8, closed_loop=True), make(8, closed_loop=True)
    for wc in (a, b):
        perturb(wc, 14)
        wc.enable_sensors(["imu", "lf_imu"])
    a.step(n_substeps=3)
    for _ in range(3):
        b.step()
    same(a, b)
    assert torch.equal(a.sensordata, b.sensordata)            # (substeps leave the last step's rows)
    for _ in range(3):
        b.step()
    rows = b.sensordata.clone()
    b.reset()
    b.reset(env_ids=[1, 2])
    torch.cuda.synchronize()
    assert torch.equal(b.sensordata, rows)                    # (reset leaves the rows alone)
    q = a.q.clone()
    q[2, 9] = float("nan")
    a.sim_step(q_tsid=q)
    torch.cuda.synchronize()
    assert int(a.info[2, 3]) & 4
    assert float(a.sensordata[2].abs().sum()) == 0            # the skipped env's rows, and only they, are zero
    others = [0, 1, 3, 4, 5, 6, 7]
    assert float(a.sensordata[others][:, :, 3:7].norm(dim=2).min()) > 0.999


@pytest.mark.parametrize("v0", [False, True])
def test_site_counts_and_all_three_features_at_once(v0):
    """S = 1 and S = 16, with external wrenches and readouts registered as well: one step against the reference"""
    n = 16
    for S in (1, 16):
        wc = make(n, v0=v0)
        rng = np.random.default_rng(S)
        sites = [(int(rng.integers(wc.NB)), rng.normal(size=3) * 0.04, unit(rng.normal(size=4))) for _ in range(S)]
        perturb(wc, 3, spread=0.2)
        wc.qpos[:, 2] -= 0.001
        wc.apply_push([3.0, -1.0, 0.5], torque=[0.0, 0.1, 0.05], body=0, env_ids=range(0, n, 2))
        wc.enable_sim_readouts()
        wc.enable_sensors(sites)
        assert tuple(wc.sensordata.shape) == (n, S, 24) and tuple(wc.framequat.shape) == (n, S, 4)
        w = teacher_forced(wc, sr.FK(wc.model), sites, 3, range(n), lambda i: wc.sim_step(teleport=False))
        assert w["ratio"] <= 1.0 and w["spare"] == 0.0, (S, w)
        assert float(wc.foot_force[:, :, 2].sum()) > 0


def test_entry_point_errors_and_python_guards():
    from tsid_control_amd._lib import TsidbError
    wc = make(4)
    N, L, h = wc.num_envs, wc._L, wc._h
    buf = torch.zeros(N, 16, 24, dtype=wc.dtype, device=wc.device)
    vp = C.c_void_p

    def call(S, body, pos, quat, out):
        body, pos, quat = np.asarray(body, np.int32), np.asarray(pos, np.float64), np.asarray(quat, np.float64)
        rc = L.tsidb_set_sensors(h, S, body.ctypes.data_as(vp), pos.ctypes.data_as(vp), quat.ctypes.data_as(vp),
                                 vp(out.data_ptr()) if out is not None else None)
        return rc, L.tsidb_last_error(h).decode()
    ident = [1.0, 0, 0, 0]
    bad = [(1, [wc.NB], [[0, 0, 0]], [ident], buf), (1, [-1], [[0, 0, 0]], [ident], buf),          # body out of range
           (1, [0], [[0, float("nan"), 0]], [ident], buf), (1, [0], [[0, 0, 0]], [[1, float("inf"), 0, 0]], buf),   # non-finite
           (1, [0], [[0, 0, 0]], [[0.0, 0, 0, 0]], buf),                                          # zero quaternion
           (17, [0] * 17, np.zeros((17, 3)), [ident] * 17, buf),                                  # more than TSIDB_MAXSITE
           (1, [0], [[0, 0, 0]], [ident], None), (0, [0], [[0, 0, 0]], [ident], buf)]             # exactly one of the two empty
    for args in bad:
        rc, msg = call(*args)
        assert rc != 0 and "tsidb_set_sensors" in msg, (args[:2], rc, msg)
    rc, _ = call(2, [0, 3], np.zeros((2, 3)), [[2.0, 0, 0, 0], [0, 0, 3.0, 0]], buf)              # (normalised on the way in)
    assert rc == 0
    wc.sim_step(teleport=False)
    torch.cuda.synchronize()
    rows = buf.view(-1)[:N * 2 * 24].view(N, 2, 24)             # (two sites: the buffer is read as [N, 2, 24])
    assert float((rows[:, :, 3:7].norm(dim=2) - 1).abs().max()) < 1e-15
    assert call(0, [0], [[0, 0, 0]], [ident], None)[0] == 0                                       # unregisters
    for kw in (dict(sites=[]), dict(sites=["imu"] * 17), dict(sites=["nose"]), dict(sites=[(wc.NB, [0, 0, 0], ident)]),
               dict(out=torch.zeros(N, 1, 23, dtype=wc.dtype, device=wc.device)),
               dict(out=torch.zeros(N, 1, 24, dtype=torch.float32, device=wc.device)),
               dict(out=torch.zeros(N, 1, 24, dtype=wc.dtype)), dict(out=np.zeros((N, 1, 24))),
               dict(sites=["imu", "lf_imu"], out=torch.zeros(N, 24, 2, dtype=wc.dtype, device=wc.device).transpose(1, 2))):
        with pytest.raises(TsidbError):
            wc.enable_sensors(**kw)
    assert wc.sensordata is None
    mine = torch.zeros(N, 3, 24, dtype=wc.dtype, device=wc.device)
    wc.enable_sensors(["imu", "lf_imu", "rf_imu"], out=mine)
    wc.step()
    torch.cuda.synchronize()
    assert wc.sensordata.data_ptr() == mine.data_ptr()
    lf, rf = foot_bodies(wc.model)
    R, p = sr.FK(wc.model).run(wc.qpos[0].cpu().numpy())      # (open loop, nearly at rest: the pose moves by micrometres)
    assert np.abs(mine[0, 1, :3].cpu().numpy() - p[lf]).max() < 1e-3 and np.abs(mine[0, 2, :3].cpu().numpy() - p[rf]).max() < 1e-3


# ---------------------------------------------------------------------------- 8. float32
def test_sensors_match_the_numpy_reference_f32():
    """the standing and lifted cases of the float64 comparison in float32, against the reference evaluated at the float32
    state and the device's own qacc.  Measured worst cases (MI355X) are recorded in DESIGN.md section 4 "Site sensors"."""
    for name, w in scenarios("f32", False, with_walking=False):
        print(f"f32 v1 {name}: pose / velocity {w['pose_vel']:.2e}, accelerometer {w['acc']:.2e} "
              f"(largest reference {w['acc_max']:.3g} m/s^2), worst error / gate {w['ratio']:.2e}")
        assert w["ratio"] <= 1.0 and w["spare"] == 0.0, (name, w)
