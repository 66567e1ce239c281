"""a second robot.  The v0 robot of the reference (robot/v0/robot.urdf + robot.srdf, 18 actuated
joints, configuration legacy/op3_conf.py; sim model robot/v0/robot.xml: 52 colliding mesh geoms on 19 bodies, condim 4,
joint damping, geom margin, actuator ranges) compiled to its own blob (assets/op3_v0.tsidb) and run through its own
builds of the oracle (liboracle_v0.so) and of the HIP library (libtsidb_v0.so): the dimensions and the tree are
per-robot compile-time constants generated from the blob, nothing in the kernels is hard-wired to the v1 robot.
CPU: the same solver-independent pins as for v1 (structure, CRBA == RNEA columns, KKT; sim: force balance at rest,
damping, torsional friction, margin).  GPU: HIP tick and sim step vs oracle on v0."""
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NQ, NV, NA = 25, 24, 18


@pytest.fixture(scope="module")
def v0():
    from oracle.oracle import Oracle, build
    from tsid_control_amd import op3_v0_conf
    from tsid_control_amd.model import ModelBlob
    from tsid_control_amd.params import pack_params
    build()
    conf = op3_v0_conf()
    blob = ModelBlob(conf.model_blob)
    orc = Oracle(blob.raw)
    params = pack_params(conf, blob.effort_limit, blob.velocity_limit)
    q = blob.q0
    t = orc.terms(q, np.zeros(NV))
    q[2] -= t["oMf"][0][11]                      # soles onto z = 0 (WalkController.py:72-79 / legacy/biped.py)
    return dict(conf=conf, blob=blob, orc=orc, params=params, q=q)


def se3vec(o):
    R = np.asarray(o[:9]).reshape(3, 3)
    return np.concatenate([o[9:], R.T.reshape(-1)])


def refs(orc, q):
    t = orc.terms(q, np.zeros(NV))
    foot_ref = np.zeros((2, 24)); foot_ref[:, 3] = foot_ref[:, 7] = foot_ref[:, 11] = 1
    return dict(com_ref=np.concatenate([t["com"], np.zeros(6)]), posture_ref=q[7:].copy(), foot_ref=foot_ref,
                contact_ref=np.stack([se3vec(t["oMf"][0]), se3vec(t["oMf"][1])]), cop_frames=t["oMf"].copy())


def test_v0_blob_and_structure(v0):
    b = v0["blob"]
    assert list(b["model_dims"]) == [19, 25, 24, 18, 19, 1, 52, 4, 1]      # NJ NQ NV NA NB sim NG condim damping
    assert len(b["pin_parent"]) == 19 and b.q0.shape == (25,) and len(b.effort_limit) == 18
    assert abs(b["pin_inertia"].reshape(19, 10)[:, 0].sum() - 2.7849874829) < 1e-9          # total mass of robot/v0/robot.urdf
    assert abs(b.q0[2] - 0.22288998) < 1e-12 and b.q0[6] == 1.0                              # robot.srdf "standing"
    t = v0["orc"].terms(v0["q"], np.zeros(NV))
    assert abs(t["mass"] - 2.7849874829) < 1e-9
    assert abs(t["oMf"][0][11]) < 1e-12 and abs(t["oMf"][1][11]) < 1e-9                       # both soles on the floor
    assert t["oMf"][0][9] * t["oMf"][1][9] < 0                                               # one foot each side


def test_v0_rigid_body_invariants(v0):
    orc = v0["orc"]
    rng = np.random.default_rng(1)
    q = v0["q"].copy()
    q[7:] += rng.uniform(-0.4, 0.4, NA)
    qt = rng.normal(size=4); q[3:7] = qt / np.linalg.norm(qt)
    v = rng.normal(0, 0.5, NV)
    t = orc.terms(q, v)
    M = t["M"]
    assert np.abs(M - M.T).max() < 1e-12 and np.linalg.eigvalsh(M).min() > 0
    h0 = orc.rnea(q, np.zeros(NV), np.zeros(NV))
    for i in range(NV):                                                                       # CRBA == RNEA columns
        e = np.zeros(NV); e[i] = 1
        assert np.abs(orc.rnea(q, np.zeros(NV), e) - h0 - M[:, i]).max() < 1e-10
    assert np.abs(orc.rnea(q, v, np.zeros(NV)) - t["h"]).max() < 1e-10
    eps = 1e-6                                                                                # CoM Jacobian by finite differences
    for i in (0, 4, 9, 17, 23):
        dq = np.zeros(NV); dq[i] = eps
        c1 = orc.terms(orc.integrate(q, dq), v)["com"]; c0 = orc.terms(orc.integrate(q, -dq), v)["com"]
        assert np.abs((c1 - c0) / (2 * eps) - t["Jcom"][:, i]).max() < 1e-6


def test_v0_qp_dimensions_and_kkt(v0):
    from test_oracle_qp import kkt_check
    orc, params = v0["orc"], v0["params"]
    rng = np.random.default_rng(2)
    r = refs(orc, v0["q"])
    for active, dims in (((1, 1), (48, 18, 152)), ((1, 0), (36, 12, 118)), ((0, 1), (36, 12, 118))):
        q = v0["q"].copy(); q[7:] += rng.uniform(-0.05, 0.05, NA)
        v = rng.normal(0, 0.1, NV)
        qp = orc.assemble(params, q, v, r["com_ref"], r["posture_ref"], r["foot_ref"], r["contact_ref"], np.array(active, np.uint8))
        assert (qp["H"].shape[0], qp["CE"].shape[0], qp["CI"].shape[0]) == dims
        sol = orc.qp_solve(qp["_raw"])
        assert sol["status"] == 0
        kkt_check(qp, sol, tol=1e-6)
    # at rest on both feet the contact forces carry the weight (joints 1e-6 off the SRDF pose: with the legs exactly
    # straight and fMin = 0 (legacy/op3_conf.py:31) the dual active-set walk ends on a degenerate tie, status 1)
    q = v0["q"].copy(); q[7:] += 1e-6 * np.arange(NA)
    qp = orc.assemble(params, q, np.zeros(NV), r["com_ref"], r["posture_ref"], r["foot_ref"], r["contact_ref"], np.array((1, 1), np.uint8))
    sol = orc.qp_solve(qp["_raw"])
    fz = sol["x"][NV:].reshape(8, 3)[:, 2].sum()
    assert sol["status"] == 0 and abs(fz - 2.7849874829 * 9.81) < 1e-2 and np.abs(sol["x"][:NV]).max() < 1e-2


def test_v0_library_exports_and_rejects_the_other_robot(v0):
    import ctypes
    from tsid_control_amd import _lib
    from tsid_control_amd.model import ModelBlob
    from tsid_control_amd.params import P_COUNT
    L0 = _lib.load_for(v0["blob"]["model_dims"])
    L1 = _lib.load_for(ModelBlob()["model_dims"])
    assert _lib.dims(L0) == (19, 25, 24, 18, 19, 1) and _lib.dims(L1) == (21, 27, 26, 20, 21, 1)
    assert _lib.dims9(L0)[6:] == (52, 4, 1) and _lib.dims9(L1)[6:] == (21, 3, 0)   # geoms, contact dimension, damping
    p = np.zeros(P_COUNT)
    h = ctypes.c_void_p()
    raw = ModelBlob().raw                        # the v1 blob handed to the v0 build: refused before any HIP call
    rc = L0.tsidb_create(raw, len(raw), p.ctypes.data_as(ctypes.c_void_p), P_COUNT, 4, 0, 0, ctypes.byref(h))
    assert rc != 0 and b"another robot" in L0.tsidb_last_error(h)
    L0.tsidb_destroy(h)


@pytest.mark.gpu
def test_v0_tick_matches_oracle_on_gpu(v0):
    """HIP-vs-oracle on the second robot: 40 env steps (tick + base teleport + sim step, the reference loop) of 32
    perturbed envs in double support, then with feet lifted (the single-support QPs)."""
    import torch
    from oracle.oracle import new_state
    from tsid_control_amd import WalkController
    n = 32
    wc = WalkController(v0["conf"], num_envs=n, device="cuda:0")
    assert (wc.NQ, wc.NV, wc.NA, wc.NOBS) == (25, 24, 18, 61) and wc.q.shape == (n, 25) and wc.rows.shape == (n, 63)
    assert float((wc.q[0].cpu() - torch.as_tensor(v0["q"])).abs().max()) < 1e-12           # reset = the oracle's standing state
    g = torch.Generator().manual_seed(5)
    wc.q[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 0.1).to(wc.device)
    wc.v[:] = (torch.randn(n, NV, generator=g, dtype=torch.float64) * 0.05).to(wc.device)
    st = new_state(n, (NQ, NV, NA))
    for k in ("q", "v", "com_ref", "posture_ref", "foot_ref", "contact_ref", "cop_frames", "contact_active", "qpos", "qvel"):
        st[k][...] = getattr(wc, k).cpu().numpy().reshape(st[k].shape)
    d = lambda t, a: float(np.abs(t.double().cpu().numpy().reshape(a.shape) - a).max())
    for i in range(40):
        if i == 20:                                # lift feet: the 36-variable single-support QP
            wc.contact_active[::2, 0] = 0
            wc.contact_active[1::4, 1] = 0
            st["contact_active"][...] = wc.contact_active.cpu().numpy()
        wc.step()
        v0["orc"].env_step_batch(wc.params, st, nthreads=8)
        assert np.array_equal(wc.status.cpu().numpy(), st["status"]), i
        assert d(wc.tau, st["tau"]) < 1e-7 and d(wc.dv, st["dv"]) < 1e-7, i
        assert d(wc.q, st["q"]) < 1e-9 and d(wc.v, st["v"]) < 1e-9 and d(wc.obs, st["obs"]) < 1e-7, i
        assert d(wc.rows[:, 61:], st["rewdone"]) < 1e-9, i
        assert np.array_equal(wc.ncon.cpu().numpy(), st["ncon"]) and np.array_equal(wc.con_pairs.cpu().numpy(), st["con_geom"]), i
        assert d(wc.qpos, st["qpos"]) < 1e-9 and d(wc.qvel, st["qvel"]) < 1e-6, i
    assert int((wc.status != 0).sum()) == 0 and int(wc.ncon.min()) >= 1
    t = wc.rbd_terms()
    ref = [v0["orc"].terms(st["q"][e], st["v"][e]) for e in range(n)]
    for key in ("M", "h", "Jcom", "Jf", "oMf", "com"):
        o = np.stack([r[key] for r in ref])
        assert d(t[key], o) < 1e-10 * max(1.0, np.abs(o).max()), key


@pytest.mark.gpu
def test_v0_rbd_terms_large_joint_angles_f64(v0):
    """test_gpu_parity.test_rbd_terms_large_joint_angles_f64 on the second robot"""
    import torch
    from tsid_control_amd import WalkController
    from test_gpu_parity import large_joint_angles
    n = 16
    wc = WalkController(v0["conf"], num_envs=n, device="cuda:0")
    g = torch.Generator().manual_seed(6)
    wc.v[:] = torch.randn(n, NV, generator=g, dtype=torch.float64).to(wc.device)
    wc.q[:, 7:] = torch.as_tensor(large_joint_angles(n, NA)).to(wc.device)
    t = wc.rbd_terms()
    q, v = wc.q.cpu().numpy(), wc.v.cpu().numpy()
    ref = [v0["orc"].terms(q[e], v[e]) for e in range(n)]
    for key in ("M", "h", "Jcom", "Jf", "oMf", "com"):
        o = np.stack([r[key] for r in ref])
        assert float(np.abs(t[key].double().cpu().numpy().reshape(o.shape) - o).max()) < 1e-12 * max(1.0, np.abs(o).max()), key


# ---------------------------------------------------------------- the v0 sim stage (robot/v0/robot.xml)
def sim_state(v0, z_lift=0.0):
    """sim state of the standing pose: qpos (wxyz, sim joint order), ctrl = the pose (servo force 0 at rest)"""
    b, q = v0["blob"], v0["q"]
    qidx = b["mj_ctrl_qidx"]
    qpos = np.zeros(NQ)
    qpos[:3] = q[:3]; qpos[2] += z_lift; qpos[3] = q[6]; qpos[4:7] = q[3:6]
    qpos[7:] = q[qidx]
    return qpos, np.zeros(NV), np.zeros(NV), q[qidx].copy()


def test_v0_sim_model_sections(v0):
    b = v0["blob"]
    gb = b["mj_geom_body"]
    assert len(gb) == 52 and gb.max() == 18 and np.all(np.diff(gb) >= 0)        # geoms grouped by body, every body has some
    assert sorted(np.bincount(gb).tolist())[-3:] == [4, 4, 12]                   # shins 2 x 2, torso 6 x 2: "visual" meshes collide too
    assert abs(b["mj_inertia"].reshape(19, 10)[:, 0].sum() - 2.76535) < 1e-3        # robot.xml's masses (the URDF's differ slightly)
    c = b["mj_contact"]
    assert (c[0], c[1], c[2], c[8], c[9], c[10]) == (0.3, 0.001, 2.0, 4.0, 0.3, 0.001)   # robot.xml:4
    assert np.all(b["mj_damping"][:6] == 0) and np.all(b["mj_damping"][6:] == 1.084)  # robot.xml:3
    assert np.all(b["mj_armature"][6:] == 0.045) and np.all(b["mj_frictionloss"][6:] == 0.03)
    r = b["mj_act_range"].reshape(18, 4)
    assert np.all(r[:, 0] == -3.141592) and np.all(r[:, 3] == 3.0) and np.all(b["mj_act_kp"] == 21.1) and np.all(b["mj_act_kv"] == 0)
    pr = b["mj_pairs"].reshape(-1, 2)
    assert len(pr) == 1044 and np.all(gb[pr[:, 0]] != gb[pr[:, 1]])               # no pair inside one body
    par = b["mj_parent"]
    assert not any(par[gb[x]] == gb[y] or par[gb[y]] == gb[x] for x, y in pr)        # parent-child filter


def test_v0_free_fall_damping_and_implicit_euler(v0):
    """joint damping as a passive force, integrated implicitly: qvel' = qvel + h (M + h B)^-1 M qacc"""
    orc, b = v0["orc"], v0["blob"]
    qpos, qvel, ws, ctrl = sim_state(v0, z_lift=1.0)
    rng = np.random.default_rng(3)
    qvel[6:] = rng.normal(0, 2.0, NA)
    v_before = qvel.copy()
    r = orc.sim_step(qpos, qvel, ctrl, ws, self_collision=False)
    assert r["rc"] == 0 and r["ncon"] == 0 and r["nefc"] == 18
    M, B, h = r["M"], np.diag(b["mj_damping"]), 0.002
    # smooth acceleration: M a = actuator - bias - B v  (kv = 0, ctrl = q: actuator force 0)
    assert np.abs(r["qfrc_actuator"]).max() < 1e-12
    assert np.abs(M @ r["qacc_smooth"] - (-r["qfrc_bias"] - B @ v_before)).max() < 1e-9
    want = v_before + h * np.linalg.solve(M + h * B, M @ r["qacc"])
    assert np.abs(qvel - want).max() < 1e-10
    assert np.abs(qvel - (v_before + h * r["qacc"])).max() > 1e-3                # and it differs from the explicit update
    assert np.array_equal(ws, r["qacc"])                                         # the warm start keeps the solver's qacc


def test_v0_actuator_ranges(v0):
    orc, b = v0["orc"], v0["blob"]
    qpos, qvel, ws, ctrl = sim_state(v0, z_lift=1.0)
    d = b["mj_act_dof"]
    c = ctrl.copy(); c[0] = 10.0; c[1] = -10.0; c[2] = ctrl[2] + 0.05; c[3] = ctrl[3] + 0.5
    r = orc.sim_step(qpos.copy(), qvel.copy(), c, ws.copy(), self_collision=False)
    f = r["qfrc_actuator"]
    assert f[d[0]] == 3.0 and f[d[1]] == -3.0                                    # ctrl clamped to +-pi, force to +-3
    assert abs(f[d[2]] - 21.1 * 0.05) < 1e-12 and f[d[3]] == 3.0                 # inside the range: kp (ctrl - q); 21.1 * 0.5 > 3


def test_v0_margin_and_resting_contact(v0):
    """contacts exist within the 1 mm margin (dist > 0), not beyond; at rest the pyramid forces carry the sim model's weight"""
    orc = v0["orc"]
    qpos, qvel, ws, ctrl = sim_state(v0)
    r0 = orc.sim_step(qpos.copy(), qvel.copy(), ctrl, ws.copy(), self_collision=False)
    low = r0["con_dist"].min()                                                   # lowest mesh vertex relative to the sole frame
    assert r0["ncon"] >= 8 and -0.002 < low < 0
    for lift, hit in ((-low + 0.0005, True), (-low + 0.0015, False)):
        q2 = qpos.copy(); q2[2] += lift
        r = orc.sim_step(q2, qvel.copy(), ctrl, ws.copy(), self_collision=False)
        assert (r["ncon"] > 0) == hit
        if hit:
            assert r["con_dist"].min() > 0 and r["con_dist"].max() <= 0.001 and r["nefc"] == 18 + 6 * r["ncon"]
            assert r["efc_force"][18:].sum() > 0                                 # inside the margin the contact already pushes
    for i in range(500):
        r = orc.sim_step(qpos, qvel, ctrl, ws, self_collision=False)
        assert r["rc"] == 0
    feet = set(np.nonzero(v0["blob"]["mj_geom_body"] == 13)[0]) | set(np.nonzero(v0["blob"]["mj_geom_body"] == 18)[0])
    assert set(r["con_geom"].tolist()) <= feet and np.all(r["con_body1"] == -1)
    assert abs(r["efc_force"][18:].sum() - 2.76535 * 9.81) < 0.3 and r["efc_force"][18:].min() >= 0
    assert np.abs(qvel).max() < 0.2


def test_v0_torsional_friction_rows(v0):
    """condim 4: rows 4, 5 of each contact are normal +- mu_t * (angular velocity about the normal).  Spinning about
    the vertical makes them differ in the braking sense; without spin they are equal."""
    orc = v0["orc"]
    qpos, qvel, ws, ctrl = sim_state(v0)
    r = orc.sim_step(qpos.copy(), qvel.copy(), ctrl, ws.copy(), self_collision=False)
    f = r["efc_force"][18:].reshape(-1, 6)
    assert np.abs(f[:, 4] - f[:, 5]).max() < 0.01                                # (not exactly at equilibrium: a small yaw acceleration)
    qv = qvel.copy(); qv[5] = 2.0                                               # yaw rate, upright base
    r = orc.sim_step(qpos.copy(), qv, ctrl, ws.copy(), self_collision=False)
    f = r["efc_force"][18:].reshape(-1, 6)
    act = f[:, 4:].max(axis=1) > 0
    assert act.any() and np.all(f[act, 5] > f[act, 4] + 0.1)                     # the "- mu_t" row carries more: torque against the spin
    gen = r["M"] @ (r["qacc"] - r["qacc_smooth"])                                # J^T f
    assert gen[5] < 0


def test_v0_self_collision_at_rest_pose(v0):
    """robot.xml's rest pose has penetrating mesh pairs that no exclude covers (the camera in the neck bracket): mj_step
    makes contacts for them, and so does the restatement"""
    orc, gb = v0["orc"], v0["blob"]["mj_geom_body"]
    qpos, qvel, ws, ctrl = sim_state(v0, z_lift=1.0)
    r = orc.sim_step(qpos, qvel, ctrl, ws, self_collision=True)
    hh = r["con_body1"] >= 0
    assert r["ncon"] == hh.sum() > 0 and r["flags"] == 0
    for c in np.nonzero(hh)[0]:
        g1, g2 = int(r["con_vert"][c]) & 0x7fff, int(r["con_geom"][c])
        assert gb[g1] == r["con_body1"][c] and gb[g2] == r["con_body2"][c] and gb[g1] != gb[g2]
        assert r["con_dist"][c] < 0.001


@pytest.mark.gpu
def test_v0_sim_step_matches_oracle_on_gpu(v0):
    """the v0 sim stage on its own: robots dropped in random self-penetrating poses and orientations (floor contacts up to
    the cap, robot<->robot contacts on both Newton paths, torsional rows, damping, clamped servos), geom / vertex lists
    bit-exact, state to the tolerance of two independent MPR runs"""
    import torch
    from tsid_control_amd import WalkController
    n = 16
    wc = WalkController(v0["conf"], num_envs=n, device="cuda:0")
    g = torch.Generator().manual_seed(11)
    wc.qpos[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 1.0).to(wc.device)
    quat = torch.randn(n, 4, generator=g, dtype=torch.float64)
    quat[: n // 2] = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64) + 0.05 * quat[: n // 2]
    wc.qpos[:, 3:7] = (quat / quat.norm(dim=1, keepdim=True)).to(wc.device)
    wc.qpos[: n // 2, 2] += 0.002
    wc.qpos[n // 2:, 2] = 0.12
    wc.qvel[:, 3:6] = (torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.5).to(wc.device)
    ctrl = np.zeros((n, NA))                          # teleport=False: no joint targets (servo force kp (0 - q), clamped to +-3)
    qpos, qvel, ws = (x.cpu().numpy().copy() for x in (wc.qpos, wc.qvel, wc.qacc_warmstart))
    d = lambda t, a: float(np.abs(t.double().cpu().numpy().reshape(a.shape) - a).max())
    n_hh = n_fl = 0
    for i in range(40):
        wc.sim_step(teleport=False)
        for e in range(n):
            r = v0["orc"].sim_step(qpos[e], qvel[e], ctrl[e], ws[e], self_collision=True)
            assert r["rc"] == 0
            want = np.full(32, -1, dtype=np.int32)
            want[:r["ncon"]] = (r["con_geom"] << 16) | r["con_vert"]
            assert np.array_equal(wc.con_pairs[e].cpu().numpy(), want), (i, e)
            assert r["flags"] == int(wc.info[e, 3]) & (8 | 16 | 32)
            n_hh += int((r["con_body1"] >= 0).sum()); n_fl += int((r["con_body1"] < 0).sum())
        # (round 3: the Newton solver keeps its factor across iterations - rank-1 row updates, tree-sparse on the device and
        #  dense in the oracle - so the two converge to the solver tolerance along slightly different iterates; over 40 steps
        #  of tumbling, self-penetrating robots that grows to ~1e-7 in qpos: 5e-7 here, contact lists stay bit-exact)
        assert d(wc.qpos, qpos) < 5e-7 and d(wc.qvel, qvel) < 1e-4, i
    assert n_hh > 200 and n_fl > 1000 and bool(torch.isfinite(wc.qpos).all())
    # joint targets beyond ctrlrange (robot.xml:5), in the air: the reference loop's teleport + ctrl map + step (main.py:192-195)
    wc2 = WalkController(v0["conf"], num_envs=n, device="cuda:0")
    qt = wc2.q.clone()
    qt[:, 2] = 1.0
    qt[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 9.0).to(wc2.device)
    qidx = v0["blob"]["mj_ctrl_qidx"]
    qn = qt.cpu().numpy()
    qpos, qvel, ws = (x.cpu().numpy().copy() for x in (wc2.qpos, wc2.qvel, wc2.qacc_warmstart))
    qpos[:, :7] = qn[:, :7]                            # (quirk F6a: xyzw copied into the wxyz slot, conf.reference_quirks)
    wc2.sim_step(teleport=True, q_tsid=qt)
    sat = 0
    for e in range(n):
        r = v0["orc"].sim_step(qpos[e], qvel[e], qn[e, qidx], ws[e], self_collision=True)
        sat += int((np.abs(qn[e, qidx]) > 3.141592).sum())
    assert sat > 10 and d(wc2.qpos, qpos) < 1e-10 and d(wc2.qvel, qvel) < 1e-8


@pytest.mark.gpu
def test_v0_closed_loop_steps_match_oracle_on_gpu(v0):
    """closed loop on v0: the tick reads the sim state, the sim is driven by the TSID torques"""
    import copy
    import torch
    from oracle.oracle import new_state
    from tsid_control_amd import WalkController
    n = 16
    conf = copy.deepcopy(v0["conf"])
    conf.closed_loop, conf.reference_quirks = True, False
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    g = torch.Generator().manual_seed(13)
    wc.qpos[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 0.06).to(wc.device)
    wc.qvel[:, 6:] = (torch.randn(n, NA, generator=g, dtype=torch.float64) * 0.05).to(wc.device)
    st = new_state(n, (NQ, NV, NA))
    for k in ("q", "v", "com_ref", "posture_ref", "foot_ref", "contact_ref", "cop_frames", "contact_active", "qpos", "qvel"):
        st[k][...] = getattr(wc, k).cpu().numpy().reshape(st[k].shape)
    d = lambda t, a: float(np.abs(t.double().cpu().numpy().reshape(a.shape) - a).max())
    for i in range(60):
        wc.step()
        v0["orc"].env_step_batch(wc.params, st, nthreads=8)
        assert np.array_equal(wc.status.cpu().numpy(), st["status"]), i
        assert np.array_equal(wc.con_pairs.cpu().numpy(), st["con_geom"]), i
        assert d(wc.tau, st["tau"]) < 1e-6 and d(wc.qpos, st["qpos"]) < 1e-8 and d(wc.qvel, st["qvel"]) < 1e-5, i
    assert bool(torch.isfinite(wc.qpos).all()) and int(wc.ncon.min()) >= 1


def test_v0_symmetric_stance_has_redundant_equalities(v0):
    """Finding: with 5 joints per leg (no ankle roll) the two rigid 6-D foot contacts of a mirror-symmetric stance are
    linearly dependent (the wrench each leg cannot resist is the mirror image of the other's: the same line), so the
    equality block has rank 17 of 18 at the SRDF pose AND at any symmetric crouch; the solver then fails - in the
    equality phase (add_constraint sees the dependent row: status 4) or, when rounding hides the dependency, as
    infeasible (status 1).  Perturbed poses (what the tests and the bench use) are regular."""
    orc, params = v0["orc"], v0["params"]
    r = refs(orc, v0["q"])
    for knee in (0.0, 0.645):
        q = v0["q"].copy()
        q[7 + 2], q[7 + 5], q[7 + 6] = 0.423 * knee, knee, 0.577 * knee          # left hip pitch / knee / ankle pitch
        q[7 + 10], q[7 + 13], q[7 + 14] = -0.423 * knee, -knee, -0.577 * knee    # right leg: mirrored axes
        rr = refs(orc, q)
        qp = orc.assemble(params, q, np.zeros(NV), rr["com_ref"], rr["posture_ref"], rr["foot_ref"], rr["contact_ref"], np.array((1, 1), np.uint8))
        sv = np.linalg.svd(qp["CE"], compute_uv=False)
        assert sv[-1] < 1e-10 * sv[0] and sv[-2] > 1e-3 * sv[0]
        assert orc.qp_solve(qp["_raw"])["status"] in (1, 4)
    # a failed QP hands nothing on: tau = dv = f = 0 (the reference stops its loop before reading the solution, main.py:122-124)
    q, v = v0["q"].copy(), np.zeros(NV)
    out = orc.tsid_tick(params, q, v, r["com_ref"], r["posture_ref"], r["foot_ref"], r["contact_ref"], np.array((1, 1), np.uint8))
    assert out["status"] in (1, 4) and not out["tau"].any() and not out["dv"].any() and not out["f"].any()
    assert np.array_equal(q, v0["q"]) and not v.any()


@pytest.mark.gpu
def test_v0_failed_tick_outputs_are_zero_and_closed_loop_stays_finite(v0):
    """half of the envs get a non-finite CoM reference: their ticks end with status 4 (deterministically, on the device as
    in the oracle), tau = dv = f = 0 and done = 1, and in the closed loop those robots go limp (held only by
    joint friction and damping) instead of being driven by whatever the solver state held; the other half keeps balancing.  (A QP that
    fails inside the solver gives the same zero outputs, but on this robot's near-singular equality block WHETHER it
    fails can depend on rounding - see test_v0_symmetric_stance_has_redundant_equalities.)"""
    import copy
    import torch
    from oracle.oracle import new_state
    from tsid_control_amd import WalkController
    n = 8
    conf = copy.deepcopy(v0["conf"])
    conf.closed_loop, conf.reference_quirks = True, False
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    g = torch.Generator().manual_seed(17)
    wc.qpos[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 0.06).to(wc.device)
    wc.com_ref[: n // 2, 1] = float("nan")
    st = new_state(n, (NQ, NV, NA))
    for k in ("q", "v", "com_ref", "posture_ref", "foot_ref", "contact_ref", "cop_frames", "contact_active", "qpos", "qvel"):
        st[k][...] = getattr(wc, k).cpu().numpy().reshape(st[k].shape)
    d = lambda t, a: float(np.abs(t.double().cpu().numpy().reshape(a.shape) - a).max())
    h = n // 2
    for i in range(90):      # (the limp robots' stick-slip amplifies rounding ~10x per 15 steps: 1e-8 after 105)
        wc.step()
        v0["orc"].env_step_batch(wc.params, st, nthreads=8)
        assert np.array_equal(wc.status.cpu().numpy(), st["status"]) and wc.status.tolist() == [4] * h + [0] * h, i
        assert float(wc.tau[:h].abs().max()) == 0 and float(wc.dv[:h].abs().max()) == 0 and float(wc.f[:h].abs().max()) == 0
        assert bool((wc.done[:h] == 1).all()) and not st["tau"][:h].any() and not st["dv"][:h].any()
        assert d(wc.tau, st["tau"]) < 1e-5 and d(wc.qpos, st["qpos"]) < 1e-7 and d(wc.qvel, st["qvel"]) < 1e-4, i   # (closed loop: rounding feeds back)
    assert bool(torch.isfinite(wc.qpos).all()) and float(wc.qpos[:, 2].min()) > 0.1
