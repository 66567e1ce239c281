"""Direct actuator control of the sim stage (tsidb_set_ctrl / tsidb_sim_ctrl; MuJoCo's mj_data.ctrl, the field a caller of
mj_step writes to drive the actuators): the three modes against the oracle's sim step from teacher-forced states, the
replay identities that tie each mode to the path it replaces, the multi-step launch, the actuator_force readout, the
input guard, reset, the C-ABI's errors and the pipelined and captured paths.

Teacher forcing: before every step the device state is copied to the oracle, both step once, the results are compared -
the device then carries on from its own result.  float64 gates are those of
test_hinge_couple_in_contact_matches_oracle_motor_torque (1e-8 on qpos, 1e-5 on qvel per step), contact lists and cap
flags bit-exact.  float32 gates: F32_GATES below."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64_GATE = (1e-8, 1e-5)
# float32 device against the float64 oracle, per teacher-forced step: each gate is 2 x the largest error the SAME comparison
# shows on the paths that existed before ctrl, from the same states, with the same number of steps and under the same drive
# (measured with measure_f32_baseline() below, ctrl never registered): teleport to the sim's own base pose + the same joint
# targets through q_tsid for "position"; the closed loop (the tick's tau as motor torques) for "motor" and "residual_closed";
# for "residual_open" the open-loop env step with the residual added to the joints of the q_tsid the sim stage is handed (the
# same targets, so the same servo forces: +-0.1 rad on kp loads the joints a hundred times harder than plain standing does).
# An (env, step) pair whose contact list differs between the float32 device and the float64 oracle (a contact at the margin on
# one side only) is left out of the state comparison; F32_MISMATCH_CAP bounds their share.
# key                      measured on the pre-ctrl path: qpos, qvel, pairs with differing contact lists     gate = 2 x
# position, v1             1.983e-03  9.916e-01    7 / 480                                                   3.966e-03  1.983e+00
# position, v0             4.516e-03  2.258e+00    0 / 480                                                   9.032e-03  4.516e+00
# motor, v1                9.409e-04  4.705e-01   14 / 480                                                   1.882e-03  9.410e-01
# motor, v0                4.514e-03  2.257e+00    0 / 480                                                   9.028e-03  4.514e+00
# residual_open, v1        1.293e-05  6.464e-03    0 / 960                                                   2.586e-05  1.293e-02
# residual_closed, v1      1.260e-07  2.620e-05    4 / 480                                                   2.520e-07  5.240e-05
# (the tumbled states are violent: robots dropped centimetres into the floor with links inside each other, contact forces of
#  hundreds of newtons on a 3 kg robot - float32 loses three digits there in one step, on the old paths as on the new ones)
F32_GATES = {
    ("position", False): (2 * 1.983e-03, 2 * 9.916e-01),
    ("position", True): (2 * 4.516e-03, 2 * 2.258e+00),
    ("motor", False): (2 * 9.409e-04, 2 * 4.705e-01),
    ("motor", True): (2 * 4.514e-03, 2 * 2.257e+00),
    ("residual_open", False): (2 * 1.293e-05, 2 * 6.464e-03),
    ("residual_closed", False): (2 * 1.260e-07, 2 * 2.620e-05),
}
F32_MISMATCH_CAP = 0.02
TUMBLE_ENVS, TUMBLE_STEPS = 24, 20
# float32 states: those of the float64 tests where the pre-ctrl teleport path keeps the contact lists of float32 and float64
# together on all but F32_MISMATCH_CAP of the steps (v0).  On v1 it does not wherever a foot lies flat on the floor: its hull
# vertices sit at the contact margin, in or out by rounding, and which of them the plane-mesh rule picks differs - measured on the
# teleport path with the upright envs of tumbled() 2 mm above, 4, 8 and 15 mm below standing height and tilted by 0.05, 0.2 and 0.4:
# 24 to 100 of 480 lists differ (of them 7 among the dropped envs); open-loop standing pressed 0 to 15 mm into the floor:
# 183 to 257 of 960.  So the v1 float32 cases start the upright envs F32_LIFT = 30 cm up (they fall 8 mm in the 20 steps: half of
# the envs in the air, the contacts are those of the dropped quarter, 1910 of them; 7 of 480 lists differ) and hold the open-loop
# base F32_OPEN_LIFT = 5 cm above the floor (the contacts are robot<->robot ones; 0 of 960 differ; at 1 cm a residual swings feet
# into the floor and 26 of 960 differ).  Feet on the floor in float32 on v1 are covered by the closed-loop residual case.
F32_LIFT = {False: 0.3, True: 0.002}      # [v0]: height of the upright envs of tumbled() above standing
F32_OPEN_LIFT = 0.05


def make(n, dtype="f64", v0=False, **over):
    from tsid_control_amd import RobotConfig, WalkController, op3_v0_conf
    conf = op3_v0_conf() if v0 else RobotConfig()
    conf.dtype = dtype
    for k, v in over.items():
        setattr(conf, k, v)
    return WalkController(conf, num_envs=n, device="cuda:0")


@pytest.fixture(scope="module")
def oracles(oracle):
    """the oracle of each robot: [False] the v1 robot's, [True] the v0 robot's"""
    from oracle.oracle import Oracle
    from tsid_control_amd import op3_v0_conf
    from tsid_control_amd.model import ModelBlob
    return {False: oracle, True: Oracle(ModelBlob(op3_v0_conf().model_blob).raw)}


SIM_STATE = ("q", "v", "tau", "dv", "f", "status", "rows", "qpos", "qvel", "qacc_warmstart", "ncon", "con_pairs", "info")


def same(a, b, keys=SIM_STATE, rows=slice(None)):
    for k in keys:
        x, y = getattr(a, k)[rows], getattr(b, k)[rows]
        assert torch.equal(x, y), (k, (x != y).nonzero()[:6].tolist())


def rand(shape, seed, wc, scale=1.0):
    """uniform in +-scale / 2, drawn on the host in float64"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5) * scale).to(wc.device, wc.dtype)


def tumbled(wc, seed=11, lift=0.002, tilt=0.05):
    """the states of test_v0_sim_step_matches_oracle_on_gpu: joints anywhere within +-0.5 rad of the standing pose (links
    penetrate each other), the first half of the envs nearly upright `lift` above their standing height (feet in contact),
    the rest in random orientations with angular velocity - dropped at 12 cm (in the floor) or, the last quarter, 1 m up in
    the air"""
    n, NA = wc.num_envs, wc.NA
    g = torch.Generator().manual_seed(seed)
    wc.qpos[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 1.0).to(wc.device, wc.dtype)
    quat = torch.randn(n, 4, generator=g, dtype=torch.float64)
    quat[: n // 2] = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64) + tilt * quat[: n // 2]
    wc.qpos[:, 3:7] = (quat / quat.norm(dim=1, keepdim=True)).to(wc.device, wc.dtype)
    wc.qpos[: n // 2, 2] += lift
    wc.qpos[n // 2:, 2] = 0.12
    wc.qpos[3 * n // 4:, 2] = 1.0
    wc.qvel[:, 3:6] = (torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.5).to(wc.device, wc.dtype)


def closed_standing(n, dtype="f64", seed=5, **over):
    """closed-loop standing (test_closed_loop_matches_oracle_and_stands), joints perturbed by +-1 cm-ish"""
    wc = make(n, dtype, closed_loop=True, **over)
    wc.qpos[:, 7:] += rand((n, wc.NQ - 7), seed, wc, 0.02)
    return wc


def perturbed(n, dtype="f64", seed=3, **over):
    """open-loop standing (test_env_loop_f64_matches_oracle): TSID joints moved by +-0.05 rad, TSID velocities N(0, 0.05)"""
    wc = make(n, dtype, **over)
    g = torch.Generator().manual_seed(seed)
    wc.q[:, 7:] += ((torch.rand(n, wc.NA, generator=g, dtype=torch.float64) - 0.5) * 0.1).to(wc.device, wc.dtype)
    wc.v[:] = (torch.randn(n, wc.NV, generator=g, dtype=torch.float64) * 0.05).to(wc.device, wc.dtype)
    return wc


def teacher_forced(wc, orc, steps, advance, drive):
    """`steps` times: copy the device's sim state to the oracle, advance() the device by one sim step, step the oracle with
    what drive() returns - (base [n, 7] or None: the pose the step teleported to, ctrl [n, NA] position targets, motor [n, NA]
    torques in TSID joint order or None), read AFTER the device step (the tick's outputs are among them).  No step may be
    skipped on either side.  Returns the largest |qpos| and |qvel| differences over the (env, step) pairs whose contact list
    and cap flags are identical on both sides, the number of pairs, of those that are not, and of contacts seen."""
    from tsid_control_amd.params import P_SELF_COLLISION
    n = wc.num_envs
    L = orc.lib
    L.or_sim_step_ext.restype = C.c_int
    L.or_model_set_plane_mesh.argtypes = [C.c_void_p, C.c_int]
    L.or_model_set_plane_mesh(orc.m, 1)
    sc = int(wc.params[P_SELF_COLLISION] != 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    host = lambda t: t.double().cpu().numpy().copy()
    out = dict(qpos=0.0, qvel=0.0, pairs=0, mismatched=0, contacts=0, mismatched_by_env=[0] * n)
    for i in range(steps):
        qpos, qvel, ws = host(wc.qpos), host(wc.qvel), host(wc.qacc_warmstart)
        advance(i)
        torch.cuda.synchronize()
        base, ctrl, motor = drive()
        got_qpos, got_qvel = host(wc.qpos), host(wc.qvel)
        pairs, info = wc.con_pairs.cpu().numpy(), wc.info.cpu().numpy()
        for e in range(n):
            qp, qv, w = qpos[e].copy(), qvel[e].copy(), ws[e].copy()
            if base is not None:
                qp[:7] = base[e]
            c = np.ascontiguousarray(ctrl[e], dtype=np.float64)
            m = np.ascontiguousarray(motor[e], dtype=np.float64) if motor is not None else None
            inf = orc.S.OrSimInfo()
            rc = L.or_sim_step_ext(orc.m, p(qp), p(qv), p(c), p(m) if m is not None else None, p(w), None, None, sc, C.byref(inf))
            assert rc == 0 and not int(info[e, 3]) & 4, (i, e, rc, int(info[e, 3]))
            want = np.full(32, -1, dtype=np.int32)
            want[:inf.ncon] = (np.array(inf.con_geom)[:inf.ncon] << 16) | np.array(inf.con_vert)[:inf.ncon]
            out["pairs"] += 1
            out["contacts"] += int(inf.ncon)
            if not np.array_equal(pairs[e], want) or inf.flags != int(info[e, 3]) & (8 | 16 | 32):
                out["mismatched"] += 1
                out["mismatched_by_env"][e] += 1
                continue
            out["qpos"] = max(out["qpos"], float(np.abs(got_qpos[e] - qp).max()))
            out["qvel"] = max(out["qvel"], float(np.abs(got_qvel[e] - qv).max()))
    return out


def gate(err, dtype, key, what):
    """float64: contact lists bit-exact, F64_GATE; float32: F32_GATES[key] on the pairs with identical contact lists, which
    must be all but F32_MISMATCH_CAP of them"""
    print(what, dtype, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in err.items()})
    if dtype == "f64":
        assert err["mismatched"] == 0, (what, err)
        tol = F64_GATE
    else:
        assert err["mismatched"] <= F32_MISMATCH_CAP * err["pairs"], (what, err)
        tol = F32_GATES[key]
    assert err["qpos"] < tol[0] and err["qvel"] < tol[1], (what, dtype, err, tol)


def position_targets(wc, v0, seed=21):
    """constant joint targets.  v0: anywhere in +-4.5 rad - a third beyond ctrlrange (+-pi), most far enough from the joint
    for forcerange (+-3 N m) to clamp the servo; v1 (no ranges, kp as in robot.xml): within +-0.3 rad of where the joints are"""
    if v0:
        return rand((wc.num_envs, wc.NA), seed, wc, 9.0).contiguous()
    return (wc.qpos[:, 7:] + rand((wc.num_envs, wc.NA), seed, wc, 0.6)).contiguous()


# ---------------------------------------------------------------------------- (1) POSITION vs the oracle
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_position_mode_matches_oracle(oracles, dtype, v0):
    """set_ctrl(targets, "position") + sim_step(teleport=False) against oracle.sim_step's ctrl argument (or_sim_step_ext
    without motor torques), 24 tumbled robots x 20 teacher-forced steps, both robots.
    float32, per step, qpos / qvel (measured on the pre-ctrl path: teleport to the sim's own base pose + the same targets
    through q_tsid; gate = 2 x): v0 4.516e-03 / 2.258 on the old path, gate 9.032e-03 / 4.516, position mode 4.516e-03 / 2.258 with
    0 of 480 contact lists differing.  v1 (upright envs 30 cm up, F32_LIFT: with feet flat on the floor the old path itself
    has 73 of 480 lists differing) 1.983e-03 / 0.9916 on the old path with 7 of 480 differing, gate 3.966e-03 / 1.983, position
    mode 1.983e-03 / 0.9916 with 7 of 480."""
    wc = make(TUMBLE_ENVS, dtype, v0)
    tumbled(wc, lift=F32_LIFT[v0] if dtype == "f32" else 0.002)
    ctrl = position_targets(wc, v0)
    if v0:
        rg = wc.model["mj_act_range"].reshape(wc.NA, 4)
        c = ctrl.double().cpu().numpy()
        assert int(((c < rg[:, 0]) | (c > rg[:, 1])).sum()) > 10
    wc.set_ctrl(ctrl, "position")
    err = teacher_forced(wc, oracles[v0], TUMBLE_STEPS, lambda i: wc.sim_step(teleport=False),
                         lambda: (None, ctrl.double().cpu().numpy(), None))
    assert err["contacts"] > 200
    gate(err, dtype, ("position", v0), f"position v0={v0}")


# ---------------------------------------------------------------------------- (2) MOTOR vs the oracle
def tsid_order(wc, ctrl):
    """[n, NA] actuator-order values -> TSID joint order (what or_sim_step_ext's motor_tau is indexed by)"""
    qidx = np.asarray(wc.model["mj_ctrl_qidx"])
    out = np.zeros_like(ctrl)
    out[:, qidx - 7] = ctrl
    return out


@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_motor_mode_matches_oracle(oracles, dtype, v0):
    """set_ctrl(torques, "motor") + sim_step(teleport=False) against or_sim_step_ext with motor_tau = the torques permuted to
    TSID joint order; random torques within +-0.4 N m, same states as the position test.
    float32, per step, qpos / qvel (measured on the pre-ctrl path: the closed-loop step whose tick supplies the torques;
    gate = 2 x): v0 4.514e-03 / 2.257 on the old path, gate 9.028e-03 / 4.514, motor mode 4.522e-03 / 2.261 with 1 of 480 contact
    lists differing.  v1 (upright envs 30 cm up, as for the position mode) 9.409e-04 / 0.4705 on the old path, gate 1.882e-03 /
    0.941, motor mode 7.457e-04 / 0.3729 with 5 of 480 differing."""
    wc = make(TUMBLE_ENVS, dtype, v0)
    tumbled(wc, lift=F32_LIFT[v0] if dtype == "f32" else 0.002)
    ctrl = rand((wc.num_envs, wc.NA), 23, wc, 0.8).contiguous()
    wc.set_ctrl(ctrl, "motor")
    c = ctrl.double().cpu().numpy()
    assert not np.array_equal(tsid_order(wc, c), c)                 # (the permutation is not the identity)
    err = teacher_forced(wc, oracles[v0], TUMBLE_STEPS, lambda i: wc.sim_step(teleport=False),
                         lambda: (None, np.zeros_like(c), tsid_order(wc, c)))
    assert err["contacts"] > 200
    gate(err, dtype, ("motor", v0), f"motor v0={v0}")


# ---------------------------------------------------------------------------- (3) RESIDUAL vs the oracle
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residual_mode_open_loop_matches_oracle(oracle, dtype):
    """open loop, step() = tick + base teleport + sim: the oracle's sim step gets the teleported base pose and
    ctrl = q[mj_ctrl_qidx] + r.  float64 tolerances of test_env_loop_f64_matches_oracle (1e-9 / 1e-6, there after 40
    free-running steps, here per teacher-forced step).  float32 (base held 5 cm above the floor, F32_OPEN_LIFT: with the
    feet teleported onto the floor every step the old path itself has 183 of 960 contact lists differing), per step, qpos /
    qvel, measured on the pre-ctrl path under the same drive - the residual added to the joints of the q_tsid handed to
    sim_step(teleport=True): 1.293e-05 / 6.464e-03 with 0 of 960 lists differing, gate 2.586e-05 / 1.293e-02; residual mode
    1.293e-05 / 6.464e-03 with 0 of 960."""
    n = 32
    wc = perturbed(n, dtype)
    if dtype == "f32":
        wc.q[:, 2] += F32_OPEN_LIFT
    r = rand((n, wc.NA), 31, wc, 0.2).contiguous()
    wc.set_ctrl(r, "residual")
    qidx = np.asarray(wc.model["mj_ctrl_qidx"])

    def drive():
        q = wc.q.double().cpu().numpy()
        return q[:, :7], q[:, qidx] + r.double().cpu().numpy(), None      # (reference_quirks: q[:7] copied as it is)

    err = teacher_forced(wc, oracle, 30, lambda i: wc.step(), drive)
    assert (err["contacts"] > 100 or dtype == "f32") and int(wc.status.abs().sum()) == 0   # (float32: held above the floor)
    print("residual open", dtype, err)
    if dtype == "f64":
        assert err["mismatched"] == 0 and err["qpos"] < 1e-9 and err["qvel"] < 1e-6, err
    else:
        gate(err, dtype, ("residual_open", False), "residual open")
    ref = perturbed(n, dtype)
    if dtype == "f32":
        ref.q[:, 2] += F32_OPEN_LIFT
    for _ in range(30):
        ref.step()
    assert not torch.equal(ref.qpos, wc.qpos)                     # (the residual did act)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residual_mode_closed_loop_matches_oracle(oracle, dtype):
    """closed loop, step() = tick on the sim state + sim driven by tau: the oracle's sim step gets motor = tau + r (r permuted
    to TSID joint order).  float64 tolerances of test_hinge_couple_in_contact_matches_oracle_motor_torque.  float32, per step,
    qpos / qvel (measured on the pre-ctrl path, the same closed-loop steps without a buffer; gate = 2 x): 1.260e-07 / 2.620e-05
    on the old path, 4 of 480 contact lists differing; gate 2.520e-07 / 5.240e-05; with the residual 1.180e-07 / 2.936e-05, 4 of
    480 - passes."""
    n = 16
    wc = closed_standing(n, dtype)
    r = rand((n, wc.NA), 33, wc, 0.3).contiguous()
    wc.set_ctrl(r, "residual")
    rt = tsid_order(wc, r.double().cpu().numpy())
    err = teacher_forced(wc, oracle, 30, lambda i: wc.step(),
                         lambda: (None, np.zeros((n, wc.NA)), wc.tau.double().cpu().numpy() + rt))
    assert err["contacts"] > 100 and int(wc.status.abs().sum()) == 0
    gate(err, dtype, ("residual_closed", False), "residual closed")


def measure_f32_baseline(oracles):
    """What F32_GATES are twice of: the comparisons above on the paths that do not read ctrl (none is registered), float32.
    Not a test; run on the GPU by hand when the gates have to be re-derived."""
    res = {}
    for v0 in (False, True):
        wc = make(TUMBLE_ENVS, "f32", v0)
        tumbled(wc, lift=F32_LIFT[v0])
        ctrl = position_targets(wc, v0)
        qidx = torch.as_tensor(np.asarray(wc.model["mj_ctrl_qidx"], dtype=np.int64), device=wc.device)
        qt = torch.zeros_like(wc.q)

        def advance(i):
            qt[:, :7] = wc.qpos[:, :7]              # (reference_quirks: copied as it is - the teleport changes nothing)
            qt[:, qidx] = ctrl
            wc.sim_step(teleport=True, q_tsid=qt)
        res["position", v0] = teacher_forced(wc, oracles[v0], TUMBLE_STEPS, advance, lambda: (None, ctrl.double().cpu().numpy(), None))
        wc = make(TUMBLE_ENVS, "f32", v0, closed_loop=True)
        tumbled(wc, lift=F32_LIFT[v0])
        res["motor", v0] = teacher_forced(wc, oracles[v0], TUMBLE_STEPS, lambda i: wc.step(),
                                          lambda: (None, np.zeros((wc.num_envs, wc.NA)), wc.tau.double().cpu().numpy()))
    wc = perturbed(32, "f32")
    wc.q[:, 2] += F32_OPEN_LIFT
    qidx = np.asarray(wc.model["mj_ctrl_qidx"])
    r = rand((32, wc.NA), 31, wc, 0.2)                  # (the residual of the test, here inside the TSID state the sim is handed)
    qt = torch.zeros_like(wc.q)

    def advance(i):
        wc.tick()
        qt.copy_(wc.q)
        qt[:, torch.as_tensor(qidx, device=wc.device).long()] += r
        wc.sim_step(teleport=True, q_tsid=qt)

    def drive():
        q = qt.double().cpu().numpy()
        return q[:, :7], q[:, qidx], None
    res["residual_open", False] = teacher_forced(wc, oracles[False], 30, advance, drive)
    wc = closed_standing(16, "f32")
    res["residual_closed", False] = teacher_forced(wc, oracles[False], 30, lambda i: wc.step(),
                                                   lambda: (None, np.zeros((16, wc.NA)), wc.tau.double().cpu().numpy()))
    return res


# ---------------------------------------------------------------------------- (4) replay identities, device vs device
def test_motor_replay_of_recorded_tau_is_bit_identical():
    """(a) a closed-loop run records tau; a second run from the same state applies ctrl_from_tau(tau_k) in motor mode before
    step k: the tick computes the same tau from the same state and the sim applies the same numbers"""
    n = 16
    a, b = closed_standing(n), closed_standing(n)
    taus = []
    for _ in range(40):
        a.step()
        taus.append(a.tau.clone())
    buf = torch.zeros(n, b.NA, dtype=b.dtype, device=b.device)
    b.set_ctrl(buf, "motor")
    for k in range(40):
        buf.copy_(b.ctrl_from_tau(taus[k]))
        b.step()
    torch.cuda.synchronize()
    same(a, b)
    assert b.ctrl is buf and float(a.qvel.abs().max()) > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_position_replay_of_the_teleport_targets_is_bit_identical(dtype):
    """(b) open-loop sim_step(teleport=True) against position mode with ctrl_from_q(q) and the same teleport"""
    n = 16
    a, b = perturbed(n, dtype, reference_quirks=False), perturbed(n, dtype, reference_quirks=False)
    buf = torch.zeros(n, b.NA, dtype=b.dtype, device=b.device)
    b.set_ctrl(buf, "position")
    for k in range(30):
        for w in (a, b):
            w.tick()
        buf.copy_(b.ctrl_from_q(b.q))
        a.sim_step(teleport=True)
        b.sim_step(teleport=True)
    torch.cuda.synchronize()
    same(a, b)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zero_residual_is_bit_identical_to_no_buffer(dtype):
    """(c) as test_zero_buffer_and_unpushed_envs_are_bit_identical does for xfrc: closed and open loop"""
    for closed in (True, False):
        a, b = (closed_standing(16, dtype) if closed else perturbed(16, dtype) for _ in range(2))
        b.set_ctrl(torch.zeros(16, b.NA, dtype=b.dtype, device=b.device), "residual")
        for _ in range(50):
            a.step(); b.step()
        torch.cuda.synchronize()
        same(a, b)


# ---------------------------------------------------------------------------- (5) sim_steps(n)
@pytest.mark.parametrize("dtype,waves", [("f64", 1), ("f64", 2), ("f32", 1), ("f32", 2)])
def test_sim_steps_equals_single_launches(dtype, waves):
    """sim_steps(n) (tsidb_sim_ctrl: up to 8 steps per launch) against n sim_step(teleport=False) launches, bit for bit - with
    the readouts and the sensors registered, whose rows are the last step's"""
    n = 16
    for steps, mode in ((1, "position"), (3, "motor"), (8, "residual"), (11, "position")):
        a, b = (make(n, dtype, sim_waves=waves) for _ in range(2))
        for w in (a, b):
            tumbled(w, seed=4)
            w.qpos[:, 2] = w.qpos[:, 2].clamp(max=0.4)
            c = rand((n, w.NA), 41, w, 0.4)
            w.set_ctrl((w.qpos[:, 7:] + c).contiguous() if mode != "motor" else c.contiguous(), mode)
            w.enable_sim_readouts()
            w.enable_sensors(["imu", "lf_imu"])
        for _ in range(steps):
            a.sim_step(teleport=False)
        b.sim_steps(steps)
        torch.cuda.synchronize()
        same(a, b, keys=("qpos", "qvel", "qacc_warmstart", "ncon", "con_pairs", "info", "con_force", "con_frame", "con_pos",
                         "actuator_force", "foot_force", "foot_cop", "sensordata"))
        assert int(a.ncon.max()) > 0 and int((a.info[:, 3] & 4).sum()) == 0


# ---------------------------------------------------------------------------- (6) actuator_force
@pytest.mark.parametrize("v0", [False, True])
def test_actuator_force_readout_is_the_applied_force(v0):
    n = 8
    wc = make(n, v0=v0)
    tumbled(wc, seed=6)
    wc.enable_sim_readouts()
    c = rand((n, wc.NA), 43, wc, 0.8).contiguous()
    wc.set_ctrl(c, "motor")
    wc.sim_step(teleport=False)
    torch.cuda.synchronize()
    assert torch.equal(wc.actuator_force, c)
    tgt = position_targets(wc, v0, seed=45)
    wc.set_ctrl(tgt, "position")
    qpos, qvel = wc.qpos.cpu().numpy().copy(), wc.qvel.cpu().numpy().copy()
    wc.sim_step(teleport=False)
    torch.cuda.synchronize()
    m = wc.model
    rg, kp, kv, dof = m["mj_act_range"].reshape(wc.NA, 4), m["mj_act_kp"], m["mj_act_kv"], np.asarray(m["mj_act_dof"])
    cc = np.clip(tgt.cpu().numpy(), rg[:, 0], rg[:, 1])
    want = np.clip(kp * (cc - qpos[:, dof + 1]) - kv * qvel[:, dof], rg[:, 2], rg[:, 3])
    got = wc.actuator_force.cpu().numpy()
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    if v0:
        assert int((np.abs(want) == 3.0).sum()) > 10
    # residual in the closed loop: tau + r
    wc = closed_standing(n)
    wc.enable_sim_readouts()
    r = rand((n, wc.NA), 47, wc, 0.2).contiguous()
    wc.set_ctrl(r, "residual")
    wc.step()
    torch.cuda.synchronize()
    assert torch.equal(wc.actuator_force, wc.ctrl_from_tau(wc.tau) + r)


# ---------------------------------------------------------------------------- (7) guards and lifecycle
def test_non_finite_ctrl_skips_that_env_only():
    n = 8
    wc, ref = closed_standing(n), closed_standing(n)
    for w in (wc, ref):
        w.set_ctrl(rand((n, w.NA), 51, w, 0.1).contiguous(), "residual")
    for _ in range(3):
        wc.step(); ref.step()
    wc.sync_sim()
    wc.ctrl[3, 5] = float("nan")
    qpos3, qvel3 = wc.qpos[3].clone(), wc.qvel[3].clone()
    wc.step(); ref.step()
    torch.cuda.synchronize()
    assert int(wc.info[3, 3]) & 4 and torch.equal(wc.qpos[3], qpos3) and torch.equal(wc.qvel[3], qvel3)
    others = [0, 1, 2, 4, 5, 6, 7]
    assert int((wc.info[others, 3] & 4).sum()) == 0
    same(wc, ref, keys=("qpos", "qvel", "tau", "q", "v"), rows=others)


def test_reset_zeroes_exactly_the_reset_rows():
    n = 8
    wc = closed_standing(n)
    c = torch.randn(n, wc.NA, dtype=wc.dtype, device=wc.device)
    wc.set_ctrl(c.clone(), "motor")
    wc.reset(env_ids=[1, 6])
    torch.cuda.synchronize()
    keep = [0, 2, 3, 4, 5, 7]
    assert float(wc.ctrl[[1, 6]].abs().max()) == 0 and torch.equal(wc.ctrl[keep], c[keep])
    wc.rows[:, wc.NOBS + 1] = 0
    wc.rows[[2, 5], wc.NOBS + 1] = 1
    wc.reset_done()
    torch.cuda.synchronize()
    keep = [0, 3, 4, 7]
    assert float(wc.ctrl[[1, 2, 5, 6]].abs().max()) == 0 and torch.equal(wc.ctrl[keep], c[keep])


def test_set_ctrl_and_sim_ctrl_errors():
    from tsid_control_amd import _lib
    from tsid_control_amd._lib import TsidbError
    n = 4
    wc = make(n)
    z = lambda *s, **kw: torch.zeros(*s, **{"dtype": wc.dtype, "device": wc.device, **kw})
    for bad in (z(n, wc.NA + 1), z(n, wc.NA, dtype=torch.float32), torch.zeros(n, wc.NA, dtype=wc.dtype), z(wc.NA, n).t(),
                np.zeros((n, wc.NA))):
        with pytest.raises(TsidbError):
            wc.set_ctrl(bad)
    with pytest.raises(TsidbError):
        wc.set_ctrl(z(n, wc.NA), mode="torque")
    assert wc.ctrl is None
    with pytest.raises(TsidbError):
        wc.sim_steps(1)                                              # nothing registered
    # the C-ABI itself, as test_api_error_behaviour calls it
    L, h = wc._L, wc._h
    err = lambda: L.tsidb_last_error(h)
    buf = z(n, wc.NA)
    vp = C.c_void_p
    st = [vp(t.data_ptr()) for t in (wc.qpos, wc.qvel, wc.qacc_warmstart)]
    for mode in (-1, 4, 99):
        assert L.tsidb_set_ctrl(h, vp(buf.data_ptr()), mode) != 0 and b"mode" in err()
    for mode in (_lib.CTRL_POSITION, _lib.CTRL_MOTOR, _lib.CTRL_RESIDUAL):
        assert L.tsidb_set_ctrl(h, None, mode) != 0 and len(err()) > 0
    assert L.tsidb_set_ctrl(h, vp(buf.data_ptr()), _lib.CTRL_OFF) != 0 and len(err()) > 0
    assert L.tsidb_sim_ctrl(h, 1, *st, None, None, None, None, None) != 0 and b"tsidb_set_ctrl" in err()
    assert L.tsidb_set_ctrl(h, vp(buf.data_ptr()), _lib.CTRL_POSITION) == 0
    for steps in (0, 9):
        assert L.tsidb_sim_ctrl(h, steps, *st, None, None, None, None, None) != 0 and b"TSIDB_MAX_SIM_BATCH" in err()
    assert L.tsidb_sim_ctrl(h, 1, None, *st[1:], None, None, None, None, None) != 0 and b"null" in err()
    assert L.tsidb_sim_ctrl(h, 8, *st, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert L.tsidb_set_ctrl(h, None, _lib.CTRL_OFF) == 0
    assert L.tsidb_sim_ctrl(h, 1, *st, None, None, None, None, None) != 0
    wc.set_ctrl(buf, "motor")
    assert wc.ctrl is buf and wc.ctrl_mode == "motor"
    wc.set_ctrl(None)
    assert wc.ctrl is None and wc.ctrl_mode is None


# ---------------------------------------------------------------------------- (8) pipelined and captured paths
@pytest.mark.parametrize("batch", [1, 8])
def test_residual_in_the_pipelined_step_equals_eager(batch):
    """a constant residual: step_pipelined() with sim batches of 1 and 8 steps + sync_sim() equals eager step(), bit for bit"""
    n = 32
    a, b = perturbed(n, reference_quirks=False), perturbed(n, reference_quirks=False, pipeline_sim_batch=batch)
    for w in (a, b):
        w.set_ctrl(rand((n, w.NA), 61, w, 0.2).contiguous(), "residual")
    for _ in range(20):
        a.step()
        b.step_pipelined()
    b.sync_sim()
    torch.cuda.synchronize()
    same(a, b)
    c = perturbed(n, reference_quirks=False)
    for _ in range(20):
        c.step()
    assert not torch.equal(a.qpos, c.qpos)                          # (the residual did act)


def test_residual_in_a_captured_graph_equals_eager():
    n = 32
    a, b = perturbed(n, reference_quirks=False), perturbed(n, reference_quirks=False)
    for w in (a, b):
        w.set_ctrl(rand((n, w.NA), 63, w, 0.2).contiguous(), "residual")
    graph = b.capture_steps(8)
    assert any(t is b.ctrl for t in graph.keep)
    for _ in range(3):
        for _ in range(8):
            a.step_pipelined()
        graph.replay()
    a.sync_sim(); b.sync_sim()
    torch.cuda.synchronize()
    same(a, b)
    c = perturbed(n, reference_quirks=False)
    for _ in range(24):
        c.step()
    a2 = perturbed(n, reference_quirks=False)
    a2.set_ctrl(a.ctrl.clone(), "residual")
    for _ in range(24):
        a2.step()
    torch.cuda.synchronize()
    same(a2, b)
    assert not torch.equal(c.qpos, b.qpos)
