"""Push recovery with the sim stage's external body wrenches (WalkController.apply_push; tsidb_set_xfrc = MuJoCo's
xfrc_applied): closed-loop standing and closed-loop walking (the configuration of test_closed_loop_walking_does_not_fall)
at N envs.  Each env gets one 100 ms push at the torso's centre of mass, of one magnitude, along +x / -x / +y / -y of
the torso's horizontal x axis ("forward" ... "right"; the batch is split evenly over magnitude x direction); reported is
the fraction of envs whose done flag stayed 0 from the push until 2 s after it ended.  Then the cost: env-steps/s of
closed-loop standing with no buffer, a registered all-zero buffer and small live pushes, alternating, median of the
repetitions.
    python tools/push_recovery.py [envs] [out.json]     (on an MI355X; default 4096 envs, profiles/push_recovery.json)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tsid_control_amd import RobotConfig, WalkController  # noqa: E402
from tsid_control_amd.walk_planner import WalkSchedule, op3_closed_loop_walking_conf, op3_walking_posture  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
OUT = sys.argv[2] if len(sys.argv) > 2 else "profiles/push_recovery.json"
MAGS = [0.0, 3.0, 5.0, 8.0, 12.0, 20.0, 35.0, 60.0]      # [N] on a 2.65 kg robot
DIRS = ["forward", "backward", "left", "right"]
PUSH_S, AFTER_S = 0.1, 2.0


def standing(n):
    conf = RobotConfig()
    conf.closed_loop = True
    return WalkController(conf, num_envs=n, device="cuda:0"), None


def walking(n):
    conf = op3_closed_loop_walking_conf(RobotConfig())
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    wc.posture_ref += torch.as_tensor(op3_walking_posture(), device=wc.device)
    lf, rf = wc.frames[0, 0, 9:11].cpu().numpy(), wc.frames[0, 1, 9:11].cpu().numpy()
    sched = WalkSchedule.from_demo_paths(n, conf, wc.device, wc.dtype, seed=1, q0_feet=(lf, rf),
                                         com0=wc.com_ref[0, :3].cpu().numpy(), foot_press=0.0, t_start=1.0)
    sched.enable_touchdown_feedback(0.6)
    return wc, sched


def sweep(kind, t_push):
    wc, sched = standing(N) if kind == "standing" else walking(N)
    dt = wc.conf.dt
    i = 0

    def tick():
        nonlocal i
        if sched is not None:
            sched.apply(wc, i * dt)
        wc.step()
        i += 1

    while i * dt < t_push:
        tick()
    fell_before = wc.done != 0
    # heading: the torso's x axis in the horizontal plane (wxyz quaternion in qpos[3:7])
    w, x, y, z = (wc.qpos[:, 3 + k].double() for k in range(4))
    fwd = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z)], dim=1)
    fwd = fwd / fwd.norm(dim=1, keepdim=True)
    left = torch.stack([-fwd[:, 1], fwd[:, 0]], dim=1)
    groups = len(MAGS) * len(DIRS)
    gid = torch.arange(N, device=wc.device) % groups
    mag = torch.as_tensor(MAGS, dtype=torch.float64, device=wc.device)[gid // len(DIRS)]
    dsel = gid % len(DIRS)
    d2 = torch.where((dsel == 0)[:, None], fwd, torch.where((dsel == 1)[:, None], -fwd, torch.where((dsel == 2)[:, None], left, -left)))
    force = torch.zeros(N, 3, dtype=torch.float64, device=wc.device)
    force[:, :2] = mag[:, None] * d2
    start = wc.qpos[:, :2].clone()
    wc.apply_push(force.to(wc.dtype), body=0)
    fell = fell_before.clone()
    for _ in range(round(PUSH_S / dt)):
        tick()
        fell |= wc.done != 0
    moved = ((wc.qpos[:, :2] - start).double() * d2).sum(dim=1)
    wc.clear_pushes()
    for _ in range(round(AFTER_S / dt)):
        tick()
        fell |= wc.done != 0
    torch.cuda.synchronize()
    table = {}
    for mi, m in enumerate(MAGS):
        row = {}
        for di, dname in enumerate(DIRS):
            sel = (gid == mi * len(DIRS) + di) & ~fell_before
            row[dname] = dict(envs=int(sel.sum()), not_done=round(float((~fell[sel]).double().mean()), 4),
                              moved_during_push_mm=round(1e3 * float(moved[sel].mean()), 2))
        table[f"{m:g} N"] = row
    return dict(workload=kind, envs=N, push_at_s=t_push, push_s=PUSH_S, after_s=AFTER_S, impulse_Ns=[m * PUSH_S for m in MAGS],
                fell_before_push=int(fell_before.sum()), recovery=table)


def throughput(steps=300, reps=3):
    wc, _ = standing(N)
    zero = torch.zeros(N, wc.NB, 6, dtype=wc.dtype, device=wc.device)
    live = torch.zeros_like(zero)
    g = torch.Generator().manual_seed(3)
    # live but small (the robots keep standing: a steady 2 N topples them, and fallen robots - many contacts, long solves -
    # would measure another workload, not the wrench)
    live[:, 0, :3] = (torch.randn(N, 3, generator=g, dtype=torch.float64) * 0.3).to(wc.device, wc.dtype)
    live[:, 14, :3] = (torch.randn(N, 3, generator=g, dtype=torch.float64) * 0.05).to(wc.device, wc.dtype)
    modes = dict(no_buffer=None, zero_buffer=zero, live_pushes=live)
    res = {k: [] for k in modes}
    done = {k: 0 for k in modes}
    for _ in range(50):
        wc.step()
    for _ in range(reps):
        for k, buf in modes.items():
            wc.set_xfrc(None)      # (a reset zeroes the registered rows: keep the live buffer out of it)
            wc.reset()
            wc.set_xfrc(None if buf is None else buf.clone())
            for _ in range(20):
                wc.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                wc.step()
            torch.cuda.synchronize()
            res[k].append(N * steps / (time.perf_counter() - t0))
            done[k] = max(done[k], int((wc.done != 0).sum()))
    med = {k: float(np.median(v)) for k, v in res.items()}
    return dict(workload="closed-loop standing, step() back to back (tick + sim)", envs=N, steps=steps, reps=reps,
                env_steps_per_s_median=med, all=res, envs_done_at_the_end=done,
                zero_vs_none=med["zero_buffer"] / med["no_buffer"] - 1, live_vs_none=med["live_pushes"] / med["no_buffer"] - 1)


if __name__ == "__main__":
    out = dict(device=torch.cuda.get_device_name(0), dtype="f64",
               standing=sweep("standing", 0.2), walking=sweep("walking", 2.0), throughput=throughput())
    text = json.dumps(out, indent=1)
    print(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
