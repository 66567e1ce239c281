"""Generates tests/golden/sim_step_bits.npz: the raw bits of the sim state after fixed, seeded runs of the sim kernel.

    python tests/golden/make_sim_step_bits.py [--parent <commit hash>] [--out FILE]

Run on a GPU at the commit whose results are to be pinned (the file records that hash); tests/test_gpu_sim_step_bits.py
then asserts that every later build reproduces the arrays bit for bit, in every shape of the sim kernel (one / two
wavefronts per env, one / eight sim steps per launch).  Only the public WalkController API is used, so the script runs
unchanged on either side of a kernel change.  The test imports CASES / VARIANTS / run_case from here: one definition of
the runs for the fixture and for the check.

Cases (per snapshot: qpos, qvel, qacc_warmstart, ncon, con_pairs, info; per case `cov`, what the run reached on its way -
COV_FIELDS, accumulated over every step of the sim_step cases and over the snapshots of the pipelined ones):
  a_walk_f64   64 float64 walkers on the seeded demo schedule, step_pipelined, snapshots after steps 300, 620, 700
               (double-support start, a touch-down window, mid-swing)
  b_selfcol    96 envs in self-penetrating joint poses U(-0.6, 0.6) (tests/test_gpu_parity.py _self_collision_poses): a
               third held in the air (robot<->robot contacts only, cross-branch pairs), a third dropped upright onto the
               floor, a third lying on it in six orientations (floor contacts up to the cap beside robot<->robot contacts,
               three and more contact groups; conf.sim_plane_mesh = "all", the contact rule that can reach the cap);
               30 sim_step(teleport=False)
  c_terrain    64 envs, randomize() with narrow terrain strips (per-env mass, friction, tilted floor, 1 cm steps),
               perturbed standing, 50 pipelined steps
  d_walk_f32   case a in float32
  e_v0_selfcol the v0 robot (libtsidb_v0.so): 16 envs tumbling in self-penetrating poses as in
               tests/test_v0_robot.py test_v0_sim_step_matches_oracle_on_gpu, 30 sim_step(teleport=False)
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FIXTURE = Path(__file__).resolve().parent / "sim_step_bits.npz"
FIELDS = ("qpos", "qvel", "qacc_warmstart", "ncon", "con_pairs", "info")
CASES = ("a_walk_f64", "b_selfcol", "c_terrain", "d_walk_f32", "e_v0_selfcol")
# shapes of the sim kernel: conf.sim_waves (0 = the library's choice: two wavefronts per env at these sizes) and
# conf.pipeline_sim_batch (0 = the default: eight sim steps per launch at these sizes; it only matters to step_pipelined)
VARIANTS = {"default": dict(), "w1_b1": dict(sim_waves=1, pipeline_sim_batch=1), "w2_b1": dict(sim_waves=2, pipeline_sim_batch=1),
            "w1_b8": dict(sim_waves=1, pipeline_sim_batch=8)}
WALK_SNAPSHOTS = (300, 620, 700)
DEV = "cuda:0"


def self_collision_poses(n, seed):
    """sim joint angles U(-0.6, 0.6) (tests/test_gpu_parity.py: _self_collision_poses)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 20, generator=g, dtype=torch.float64) - 0.5) * 1.2


COV_FIELDS = ("ncon_max", "flags_or", "hull_pair_contacts", "floor_contact_bodies_max", "cross_branch_contacts", "newton_iters_max")


class Coverage:
    """what a run reached: the most contacts of an env, the OR of the flag bits (info[:, 3]), robot<->robot contacts, the most
    bodies with floor contacts in one env (contact groups of the Hessian build), robot<->robot contacts between two branches
    of the tree (dense Newton factor), the most Newton iterations"""

    def __init__(self, wc):
        self.gb = np.asarray(wc.model["mj_geom_body"])
        par = np.asarray(wc.model["mj_parent"])
        anc = lambda b: {b} | (anc(int(par[b])) if par[b] >= 0 else set())
        self.anc = [anc(b) for b in range(len(par))]
        self.v = np.zeros(len(COV_FIELDS), dtype=np.int64)

    def add(self, wc):
        wc.sync_sim()
        ncon, pairs, info = wc.ncon.cpu().numpy(), wc.con_pairs.cpu().numpy(), wc.info.cpu().numpy()
        hull = (pairs >= 0) & ((pairs & 0x8000) != 0)
        groups = max(len({int(self.gb[p >> 16]) for p in row if p >= 0 and not p & 0x8000}) for row in pairs)
        cross = 0
        for p in pairs[hull]:
            a, b = int(self.gb[p & 0x7fff]), int(self.gb[p >> 16])
            cross += int(a not in self.anc[b] and b not in self.anc[a])
        v = self.v
        v[0] = max(v[0], int(ncon.max())); v[1] |= int(np.bitwise_or.reduce(info[:, 3])); v[2] += int(hull.sum())
        v[3] = max(v[3], groups); v[4] += cross; v[5] = max(v[5], int(info[:, 2].max()))


def _snap(wc, cov):
    cov.add(wc)
    torch.cuda.synchronize()
    return {k: getattr(wc, k).cpu().numpy().copy() for k in FIELDS}


def _conf(dtype, over, v0=False):
    from tsid_control_amd import RobotConfig
    if v0:
        from tsid_control_amd import op3_v0_conf
        conf = op3_v0_conf()
    else:
        conf = RobotConfig()
    conf.dtype = dtype
    for k, v in over.items():
        setattr(conf, k, v)
    return conf


def _walk(dtype, over):
    from tsid_control_amd import WalkController
    from tsid_control_amd.walk_planner import WalkSchedule, op3_walking_conf, op3_walking_posture
    n = 64
    conf = _conf(dtype, over)
    op3_walking_conf(conf)
    conf.reference_quirks = False
    wc = WalkController(conf, num_envs=n, device=DEV)
    wc.posture_ref += torch.as_tensor(op3_walking_posture(), device=wc.device).to(wc.dtype)
    lf, rf = wc.frames[0, 0, 9:11].cpu().numpy(), wc.frames[0, 1, 9:11].cpu().numpy()
    sched = WalkSchedule.from_demo_paths(n, conf, wc.device, wc.dtype, seed=1, q0_feet=(lf, rf),
                                         com0=wc.com_ref[0, :3].double().cpu().numpy())
    out, cov = [], Coverage(wc)
    for i in range(max(WALK_SNAPSHOTS)):
        wc.step_pipelined(walk=(sched, i * conf.dt))
        if i + 1 in WALK_SNAPSHOTS:
            out.append(_snap(wc, cov))
    return out, cov.v


def _selfcol(over):
    from tsid_control_amd import WalkController
    n = 96
    wc = WalkController(_conf("f64", dict(self_collision=True, sim_plane_mesh="all", **over)), num_envs=n, device=DEV)
    dev, dt = wc.device, wc.dtype
    wc.qpos[:, 7:] = self_collision_poses(n, 3).to(dev, dt)
    up = torch.tensor([1.0, 0, 0, 0], dtype=dt, device=dev)
    wc.qpos[:32, 3:7] = up          # in the air
    wc.qpos[:32, 2] = 1.0
    wc.qpos[32:64, 3:7] = up        # dropped upright: both soles and whatever the pose brings down
    wc.qpos[32:64, 2] += 0.002
    quats = torch.tensor([[0.7071068, 0.7071068, 0, 0], [0.7071068, 0, 0.7071068, 0], [0.5, 0.5, 0.5, 0.5],
                          [0.9238795, 0.3826834, 0, 0], [0.7071068, -0.7071068, 0, 0], [0.0, 1.0, 0, 0]], dtype=dt, device=dev)
    wc.qpos[64:, 3:7] = quats[torch.arange(32, device=dev) % 6]   # lying on the floor
    wc.qpos[64:, 2] = 0.03
    cov = Coverage(wc)
    for _ in range(29):
        wc.sim_step(teleport=False)
        cov.add(wc)
    wc.sim_step(teleport=False)
    return [_snap(wc, cov)], cov.v


def _terrain(over):
    from tsid_control_amd import WalkController
    n = 64
    wc = WalkController(_conf("f64", dict(reference_quirks=False, **over)), num_envs=n, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(17)
    wc.q[:, 7:] += ((torch.rand(n, 20, generator=g, dtype=torch.float64) - 0.5) * 0.1).to(wc.device, wc.dtype)
    wc.v[:] = (torch.randn(n, 26, generator=g, dtype=torch.float64) * 0.05).to(wc.device, wc.dtype)
    wc.randomize(seed=5, step_length=(0.02, 0.06))
    cov = Coverage(wc)
    for _ in range(50):
        wc.step_pipelined()
    return [_snap(wc, cov)], cov.v


def _v0(over):
    from tsid_control_amd import WalkController
    n, NA = 16, 18
    wc = WalkController(_conf("f64", over, v0=True), num_envs=n, device=DEV)
    g = torch.Generator().manual_seed(11)
    wc.qpos[:, 7:] += ((torch.rand(n, NA, generator=g, dtype=torch.float64) - 0.5) * 1.0).to(wc.device)
    quat = torch.randn(n, 4, generator=g, dtype=torch.float64)
    quat[: n // 2] = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64) + 0.05 * quat[: n // 2]
    wc.qpos[:, 3:7] = (quat / quat.norm(dim=1, keepdim=True)).to(wc.device)
    wc.qpos[: n // 2, 2] += 0.002
    wc.qpos[n // 2:, 2] = 0.12
    wc.qvel[:, 3:6] = (torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.5).to(wc.device)
    cov = Coverage(wc)
    for _ in range(29):
        wc.sim_step(teleport=False)
        cov.add(wc)
    wc.sim_step(teleport=False)
    return [_snap(wc, cov)], cov.v


def run_case(case, variant="default"):
    """(list of snapshots (dict field -> array), coverage vector) of one case in one shape of the sim kernel"""
    over = dict(VARIANTS[variant])
    if case == "a_walk_f64":
        return _walk("f64", over)
    if case == "d_walk_f32":
        return _walk("f32", over)
    if case == "b_selfcol":
        return _selfcol(over)
    if case == "c_terrain":
        return _terrain(over)
    if case == "e_v0_selfcol":
        return _v0(over)
    raise KeyError(case)


def pipelined(case):
    """cases that run step_pipelined: the only ones conf.pipeline_sim_batch changes the launches of"""
    return case in ("a_walk_f64", "c_terrain", "d_walk_f32")


def variants_of(case):
    return [v for v in VARIANTS if pipelined(case) or VARIANTS[v].get("pipeline_sim_batch", 0) <= 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="unknown", help="hash of the commit the fixture is generated at")
    ap.add_argument("--out", default=str(FIXTURE))
    a = ap.parse_args()
    arrs = {"parent_commit": np.frombuffer(a.parent.encode(), dtype=np.uint8)}
    for case in CASES:
        ref, cov = run_case(case, "default")
        for v in variants_of(case)[1:]:   # the shapes agree with each other already: the fixture holds one copy
            other, _ = run_case(case, v)
            diff = [(s, k) for s, (x, y) in enumerate(zip(ref, other)) for k in FIELDS
                    if not np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8))]
            print(f"{case}: variant {v} {'!=' if diff else '=='} default {diff}", flush=True)
            if diff:   # a shape that rounds differently at the generating commit gets a copy of its own ("case@variant/...")
                for s, snap in enumerate(other):
                    for k in FIELDS:
                        arrs[f"{case}@{v}/{s}/{k}"] = snap[k]
        for s, snap in enumerate(ref):
            for k in FIELDS:
                arrs[f"{case}/{s}/{k}"] = snap[k]
        arrs[f"{case}/cov"] = cov
        print(case, dict(zip(COV_FIELDS, cov.tolist())), flush=True)
    np.savez_compressed(a.out, **arrs)
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes at", a.parent)


if __name__ == "__main__":
    main()
