"""External body wrenches of the sim stage (tsidb_set_xfrc; MuJoCo's mj_data.xfrc_applied, the field a caller of mj_step
writes to push the robot, main.py:192-195): no behaviour change without them, the spatial-force conversion against an
independent computation (a uniform acceleration field, generalized forces J_b^T w_b from a numpy forward kinematics of the
blob, a couple against motor torques in the oracle), push recovery, reset, the pipelined and captured paths and the input
guard."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make(n, dtype="f64", v0=False, **over):
    from tsid_control_amd import RobotConfig, WalkController, op3_v0_conf
    conf = op3_v0_conf() if v0 else RobotConfig()
    conf.dtype = dtype
    for k, v in over.items():
        setattr(conf, k, v)
    return WalkController(conf, num_envs=n, device="cuda:0")


def closed_standing(n, dtype="f64", seed=5, **over):
    """closed-loop standing (test_closed_loop_matches_oracle_and_stands), joints perturbed by +-1 cm-ish"""
    wc = make(n, dtype, closed_loop=True, **over)
    g = torch.Generator().manual_seed(seed)
    wc.qpos[:, 7:] += ((torch.rand(n, wc.NQ - 7, generator=g, dtype=torch.float64) - 0.5) * 0.02).to(wc.device, wc.dtype)
    return wc


SIM_STATE = ("q", "v", "tau", "dv", "f", "status", "rows", "qpos", "qvel", "qacc_warmstart", "ncon", "con_pairs", "info")


def same(a, b, keys=SIM_STATE, rows=slice(None)):
    for k in keys:
        x, y = getattr(a, k)[rows], getattr(b, k)[rows]
        assert torch.equal(x, y), (k, (x != y).nonzero()[:6].tolist())


# ---------------------------------------------------------------------------- forward kinematics of the blob (numpy)
class FK:
    """The sim tree of the blob's mj_* sections: R_b = R_parent mj_R[b] Rz(theta_b), p_b = p_parent + R_parent pos_b,
    c_b = p_b + R_b ipos_b (tsidb_sim.hpp's kinematics, written out here independently)."""

    def __init__(self, blob):
        self.NB = int(blob["model_dims"][4])
        self.parent = blob["mj_parent"].copy()
        self.pos = blob["mj_pos"].reshape(self.NB, 3)
        self.Rq = np.stack([self.quat(q) for q in blob["mj_quat"].reshape(self.NB, 4)])
        self.inertia = blob["mj_inertia"].reshape(self.NB, 10)

    @staticmethod
    def quat(q):
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    def run(self, qpos, R0=None):
        R, p = np.zeros((self.NB, 3, 3)), np.zeros((self.NB, 3))
        R[0] = self.quat(qpos[3:7]) if R0 is None else R0
        p[0] = qpos[:3]
        for b in range(1, self.NB):
            a = self.parent[b]
            c, s = np.cos(qpos[6 + b]), np.sin(qpos[6 + b])
            R[b] = R[a] @ self.Rq[b] @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
            p[b] = p[a] + R[a] @ self.pos[b]
        com = p + np.einsum("bij,bj->bi", R, self.inertia[:, 1:4])
        return R, p, com

    def jacobians(self, qpos, eps=1e-6):
        """J [NB, 6, NV]: velocity of each body's centre of mass (world) and its angular velocity (world) per unit qvel,
        by central differences (free joint: linear dofs world frame, angular dofs body frame)"""
        NV = len(qpos) - 1
        R0 = self.quat(qpos[3:7])
        Rc, _, _ = self.run(qpos)
        J = np.zeros((self.NB, 6, NV))
        for k in range(NV):
            out = []
            for sgn in (1.0, -1.0):
                q = qpos.copy()
                r0 = None
                if k < 3:
                    q[k] += sgn * eps
                elif k < 6:
                    w = np.zeros(3)
                    w[k - 3] = sgn * eps
                    th = np.linalg.norm(w)
                    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
                    r0 = R0 @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
                else:
                    q[k + 1] += sgn * eps
                out.append(self.run(q, r0))
            (Rp, _, cp), (Rm, _, cm) = out
            J[:, :3, k] = (cp - cm) / (2 * eps)
            W = np.einsum("bij,bkj->bik", Rp - Rm, Rc) / (2 * eps)
            J[:, 3:, k] = 0.5 * np.stack([W[:, 2, 1] - W[:, 1, 2], W[:, 0, 2] - W[:, 2, 0], W[:, 1, 0] - W[:, 0, 1]], axis=1)
        return J


def lifted(wc, seed, spread=0.6):
    """in the air (1 m up), joints moved by up to +-spread / 2 (a generic configuration), at rest"""
    g = torch.Generator().manual_seed(seed)
    wc.qpos[:, 2] += 1.0
    wc.qpos[:, 7:] += ((torch.rand(wc.num_envs, wc.NQ - 7, generator=g, dtype=torch.float64) - 0.5) * spread).to(wc.device, wc.dtype)
    wc.qpos[:, 7:] = wc.qpos[:1, 7:]      # every env the same state


# ---------------------------------------------------------------------------- (a) no behaviour change
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zero_buffer_and_unpushed_envs_are_bit_identical(dtype):
    for closed in (True, False):
        a, b, c = (closed_standing(16, dtype) if closed else make(16, dtype) for _ in range(3))
        b.set_xfrc(torch.zeros(16, b.NB, 6, dtype=b.dtype, device=b.device))
        pushed = torch.arange(0, 16, 2, device=c.device)
        c.apply_push([4.0, -2.0, 1.0], torque=[0.0, 0.1, 0.0], body=0, env_ids=pushed)
        c.apply_push([0.0, 1.5, 0.5], body=14, env_ids=pushed)
        for _ in range(50):
            a.step(); b.step(); c.step()
        torch.cuda.synchronize()
        same(a, b)
        same(a, c, rows=slice(1, None, 2))
        assert not torch.equal(a.qpos[0::2], c.qpos[0::2])


# ---------------------------------------------------------------------------- (b) uniform acceleration field
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f32", False), ("f64", True), ("f32", True)])
def test_uniform_field_shifts_only_the_base_acceleration(dtype, v0):
    """F_b = mass_scale m_b a at every body, no torque: qacc changes by exactly (a, 0, ..., 0) - the columns of M of the
    world-frame translational dofs are sum_b J_b^T m_b (armature and damping sit on hinge dofs only) - so one step
    changes qvel by (dt a, 0, ..., 0), also through the damped implicit Euler of the v0 library ((M + h B) e = M e).
    Bounds: f64 1e-12 absolute; f32 5 % of |dt a| (the float32 factorisation of M; a wrong sign, frame or point of
    application is off by 100 % or more)."""
    n = 4
    wc = make(n, dtype, v0=v0, sim_frictionloss_scale=0.0, self_collision=False)     # (no constraint rows at all)
    wc.set_env_params(mass_scale=torch.full((n,), 1.1, dtype=torch.float64))
    lifted(wc, 3, spread=0.0)       # (the standing joint angles: no servo force, the accelerations stay small)
    a = torch.tensor([[0.0, 0.0, 0.0], [15.0, -10.0, 25.0], [-20.0, 5.0, 0.0], [2.5, 30.0, -10.0]], dtype=wc.dtype, device=wc.device)
    m = wc.body_masses()
    w = torch.zeros(n, wc.NB, 6, dtype=wc.dtype, device=wc.device)
    w[:, :, :3] = m[:, :, None] * a[:, None, :]
    wc.set_xfrc(w)
    v_before = wc.qvel.clone()
    wc.sim_step(teleport=False)
    torch.cuda.synchronize()
    assert int(wc.ncon.max()) == 0 and int((wc.info[:, 3] & 4).sum()) == 0
    dv = (wc.qvel - v_before).double()
    dv = dv[1:] - dv[:1]                    # against env 0 (no push, same state)
    want = wc.conf.dt * a[1:].double()
    tol_lin = 1e-12 if dtype == "f64" else 0.05 * float(want.norm(dim=1).min())
    tol_rot = 1e-12 if dtype == "f64" else 0.05 * float(want.norm(dim=1).min())
    assert float((dv[:, :3] - want).abs().max()) < tol_lin, (dv[:, :3] - want)
    assert float(dv[:, 3:].abs().max()) < tol_rot, float(dv[:, 3:].abs().max())


# ---------------------------------------------------------------------------- (c) general wrenches: J_b^T w_b
def test_general_wrenches_against_numpy_jacobians(oracle, blob):
    """Random forces and torques on random bodies, in the air without constraint rows (ncon == 0: qacc is linear in the
    wrench): delta qacc = M^-1 sum_b J_b^T w_b with M from the oracle and J_b by central differences of a numpy forward
    kinematics.  Relative error bound 1e-6 (the differences)."""
    n = 6
    wc = make(n, sim_frictionloss_scale=0.0, self_collision=False)
    lifted(wc, 11)
    wc.qvel[:] = (torch.randn(1, wc.NV, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 0.3).to(wc.device)
    rng = np.random.default_rng(7)
    w = np.zeros((n, wc.NB, 6))
    for e in range(1, n):
        for b in rng.choice(wc.NB, size=3, replace=False):
            w[e, b, :3] = rng.normal(size=3) * 2.0
            w[e, b, 3:] = rng.normal(size=3) * 0.1
    qpos, qvel = wc.qpos[0].cpu().numpy().copy(), wc.qvel[0].cpu().numpy().copy()
    wc.set_xfrc(torch.as_tensor(w, device=wc.device).contiguous())
    wc.sim_step(teleport=False)
    torch.cuda.synchronize()
    assert int(wc.ncon.max()) == 0
    qacc = wc.qacc_warmstart.cpu().numpy()          # (the step writes its qacc as the next warm start)
    M = oracle.sim_step(qpos.copy(), qvel.copy(), np.zeros(20), np.zeros(wc.NV), self_collision=False)["M"]
    J = FK(blob).jacobians(qpos)
    for e in range(1, n):
        Q = np.einsum("bik,bi->k", J, w[e])
        want = np.linalg.solve(M, Q)
        got = qacc[e] - qacc[0]
        assert np.abs(got - want).max() < 1e-6 * np.abs(want).max(), (e, np.abs(got - want).max(), np.abs(want).max())


# ---------------------------------------------------------------------------- (d) couples in contact vs the oracle
def test_hinge_couple_in_contact_matches_oracle_motor_torque(oracle, blob):
    """A couple +-tau axis_j on the child body of hinge j and on its parent is a generalized force tau on that hinge alone:
    the closed-loop step with it equals the oracle's sim step (or_sim_step_ext) with motor torques tau + tau_j e_j, both
    feet in contact.  Tolerances of test_closed_loop_matches_oracle_and_stands."""
    from tsid_control_amd.params import P_SELF_COLLISION
    n = 8
    wc = closed_standing(n)
    for _ in range(20):
        wc.step()
    fk = FK(blob)
    act_dof, ctrl_qidx = blob["mj_act_dof"], blob["mj_ctrl_qidx"]
    bodies = [3, 5, 2, 9, 14, 17, 19, 6]                  # knees, ankles, a hip, arms, the neck, a foot
    tau_j = np.array([0.3, -0.2, 0.25, -0.3, 0.15, -0.1, 0.1, 0.2])
    L = oracle.lib
    L.or_sim_step_ext.restype = C.c_int
    sc = int(wc.params[P_SELF_COLLISION] != 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for step in range(4):
        qpos, qvel, ws = (x.cpu().numpy().copy() for x in (wc.qpos, wc.qvel, wc.qacc_warmstart))
        w = torch.zeros(n, wc.NB, 6, dtype=wc.dtype, device=wc.device)
        for e in range(n):
            b = bodies[e]
            R, _, _ = fk.run(qpos[e])
            axis = R[b][:, 2]
            w[e, b, 3:] = torch.as_tensor(tau_j[e] * axis)
            w[e, fk.parent[b], 3:] = torch.as_tensor(-tau_j[e] * axis)
        wc.set_xfrc(w)
        wc.step()
        torch.cuda.synchronize()
        assert int(wc.ncon.min()) >= 2 and int(wc.status.abs().sum()) == 0
        tau = wc.tau.cpu().numpy()
        for e in range(n):
            b = bodies[e]
            lane = int(np.nonzero(act_dof == 5 + b)[0][0])
            motor = tau[e].copy()
            motor[ctrl_qidx[lane] - 7] += tau_j[e]
            qp, qv, wse = qpos[e].copy(), qvel[e].copy(), ws[e].copy()
            info = oracle.S.OrSimInfo()
            rc = L.or_sim_step_ext(oracle.m, p(qp), p(qv), p(np.zeros(20)), p(motor), p(wse), None, None, sc, C.byref(info))
            assert rc == 0 and info.ncon == int(wc.ncon[e])
            assert np.abs(wc.qpos[e].cpu().numpy() - qp).max() < 1e-8, (step, e)
            assert np.abs(wc.qvel[e].cpu().numpy() - qv).max() < 1e-5, (step, e)


# ---------------------------------------------------------------------------- (e) push recovery
# magnitudes from tools/push_recovery.py (profiles/push_recovery.json, closed-loop standing, 100 ms torso pushes, 4096 envs):
# 3 N - every env of every direction stands; 5 N - the left pushes fall; 8 N and more - every env falls
SMALL_PUSH, LARGE_PUSH = 3.0, 20.0


def test_push_recovery_behaviour():
    """256 closed-loop standing envs; 100 ms torso pushes forward, backward and sideways: the pushed envs move in the
    push direction during the push; a small push leaves every env standing (done == 0 for 2 s) and back within 5 cm of
    where it stood; a large one brings most of them down."""
    n = 256
    dirs = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]], dtype=torch.float64)
    for mag, small in ((SMALL_PUSH, True), (LARGE_PUSH, False)):
        wc = closed_standing(n, seed=9)
        for _ in range(50):
            wc.step()
        start = wc.qpos[:, :2].clone()
        d = dirs[torch.arange(n) % 4].to(wc.device, wc.dtype)
        wc.apply_push(mag * d, body=0)
        for _ in range(25):
            wc.step()
        moved = ((wc.qpos[:, :2] - start) * d[:, :2]).sum(dim=1)
        assert float(moved.min()) > 0 and float(((wc.qvel[:, :3] * d).sum(dim=1)).min()) > 0
        for _ in range(25):
            wc.step()
        wc.clear_pushes()
        fell = torch.zeros(n, dtype=torch.bool, device=wc.device)
        for _ in range(1000):
            wc.step()
            fell |= wc.done != 0
        if small:
            assert not bool(fell.any())
            assert float((wc.qpos[:, :2] - start).norm(dim=1).max()) < 0.05
        else:
            assert float(fell.double().mean()) > 0.5


# ---------------------------------------------------------------------------- (f) reset
def test_reset_zeroes_exactly_the_reset_rows():
    n = 8
    wc = closed_standing(n)
    w = torch.randn(n, wc.NB, 6, dtype=wc.dtype, device=wc.device)
    wc.set_xfrc(w.clone())
    wc.reset(env_ids=[1, 6])
    torch.cuda.synchronize()
    keep = [0, 2, 3, 4, 5, 7]
    assert float(wc.xfrc[[1, 6]].abs().max()) == 0 and torch.equal(wc.xfrc[keep], w[keep])
    wc.rows[:, wc.NOBS + 1] = 0
    wc.rows[[2, 5], wc.NOBS + 1] = 1
    wc.reset_done()
    torch.cuda.synchronize()
    keep = [0, 3, 4, 7]
    assert float(wc.xfrc[[1, 2, 5, 6]].abs().max()) == 0 and torch.equal(wc.xfrc[keep], w[keep])


# ---------------------------------------------------------------------------- (g) pipelines
@pytest.mark.parametrize("batch", [1, 8])
def test_limb_push_in_the_pipelined_step_equals_eager(batch):
    """open loop (the torso is teleported, pushes on limbs act): step_pipelined() with sim batches of 1 and 8 steps and
    eager step() give the same results, bit for bit, with a push changed half way (after sync_sim, in place)"""
    a, b = make(32, reference_quirks=False), make(32, reference_quirks=False, pipeline_sim_batch=batch)
    for w in (a, b):
        w.apply_push([0.0, 3.0, 1.0], body=14, env_ids=range(0, 32, 3))
        w.apply_push([1.0, 0.0, 0.0], torque=[0.0, 0.0, 0.05], body=6, env_ids=range(1, 32, 3))
    for i in range(20):
        if i == 11:
            for w in (a, b):
                w.sync_sim()
                w.xfrc[:, 14, 1] *= -1.0
        a.step()
        b.step_pipelined()
    b.sync_sim()
    torch.cuda.synchronize()
    same(a, b)
    c = make(32, reference_quirks=False)
    for _ in range(20):
        c.step()
    assert not torch.equal(a.qpos[0], c.qpos[0]) and torch.equal(a.qpos[2], c.qpos[2])


def test_limb_push_in_a_captured_graph_equals_eager():
    a, b = make(32, reference_quirks=False), make(32, reference_quirks=False)
    for w in (a, b):
        w.apply_push([0.0, -2.5, 1.0], body=17, env_ids=range(0, 32, 2))
    graph = b.capture_steps(8)
    for r in range(4):
        if r == 2:                                          # rewritten in place between replays: takes effect
            for w in (a, b):
                w.sync_sim()
                w.xfrc[:, 17, 2] = 4.0
        for _ in range(8):
            a.step_pipelined()
        graph.replay()
    a.sync_sim(); b.sync_sim()
    torch.cuda.synchronize()
    same(a, b)
    c = make(32, reference_quirks=False)
    c.apply_push([0.0, -2.5, 1.0], body=17, env_ids=range(0, 32, 2))
    for _ in range(32):
        c.step_pipelined()
    c.sync_sim()
    torch.cuda.synchronize()
    assert not torch.equal(c.qpos, b.qpos)                 # (the rewrite did act)


# ---------------------------------------------------------------------------- (h) errors and non-finite input
def test_set_xfrc_errors_and_non_finite_wrench():
    from tsid_control_amd._lib import TsidbError
    n = 8
    wc, ref = closed_standing(n), closed_standing(n)
    z = lambda *s, **kw: torch.zeros(*s, **{"dtype": wc.dtype, "device": wc.device, **kw})
    for bad in (z(n, wc.NB + 1, 6), z(n, wc.NB, 6, dtype=torch.float32), torch.zeros(n, wc.NB, 6, dtype=wc.dtype),
                z(n, 6, wc.NB).transpose(1, 2), np.zeros((n, wc.NB, 6))):
        with pytest.raises(TsidbError):
            wc.set_xfrc(bad)
    assert wc.xfrc is None
    for _ in range(3):
        wc.step(); ref.step()
    wc.set_xfrc(z(n, wc.NB, 6))
    wc.xfrc[3, 5, 1] = float("nan")
    qpos3 = wc.qpos[3].clone()
    wc.step(); ref.step()
    torch.cuda.synchronize()
    assert int(wc.info[3, 3]) & 4 and torch.equal(wc.qpos[3], qpos3)
    others = [0, 1, 2, 4, 5, 6, 7]
    same(wc, ref, keys=("qpos", "qvel", "tau", "q", "v"), rows=others)
    wc.set_xfrc(None)
    assert wc.xfrc is None
