"""Sim-stage readouts (WalkController.enable_sim_readouts; tsidb_set_sim_readouts = mj_data.contact, mj_contactForce,
mj_data.actuator_force): what they cost and what they show.
  cost      env-steps/s with the readouts off and on: two identically built controllers stepped over the same steps of the
            episode, timed windows of ~1 s alternating between them, closed-loop standing (step() back to back) and open-loop
            walking, the headline workload (bench.py's loop: step_pipelined() with the walking reference update in the tick,
            on WalkController.tick_stream)
  realised  the sim's centre of pressure (sim_cop) against TSID's (get_cop, double support only) and the sim's sole forces
            against TSID's planned contact forces f (the four corner forces of each sole summed), in closed-loop standing and
            closed-loop walking (tools/push_recovery.py's walking configuration)
    python tools/sim_readouts.py [envs] [out.json] [--cost-only]     (on an MI355X; default 4096 envs, profiles/sim_readouts.json)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tsid_control_amd import RobotConfig, WalkController  # noqa: E402
from tsid_control_amd.walk_planner import (WalkSchedule, op3_closed_loop_walking_conf, op3_walking_conf,  # noqa: E402
                                           op3_walking_posture)

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
COST_ONLY = "--cost-only" in sys.argv[1:]     # (the cost measurement alone: for a rocprofv3 --kernel-trace --stats run)
N = int(ARGS[0]) if len(ARGS) > 0 else 4096
OUT = ARGS[1] if len(ARGS) > 1 else "profiles/sim_readouts.json"


def walker(conf, n, touchdown=False):
    wc = WalkController(conf, num_envs=n, device="cuda:0")
    wc.posture_ref += torch.as_tensor(op3_walking_posture(), device=wc.device).to(wc.dtype)
    lf, rf = wc.frames[0, 0, 9:11].cpu().numpy(), wc.frames[0, 1, 9:11].cpu().numpy()
    sched = WalkSchedule.from_demo_paths(n, conf, wc.device, wc.dtype, seed=1, q0_feet=(lf, rf),
                                         com0=wc.com_ref[0, :3].cpu().numpy(), foot_press=0.0, t_start=1.0)
    if touchdown:
        sched.enable_touchdown_feedback(0.6)
    return wc, sched


def controller(kind):
    if kind == "standing":
        conf = RobotConfig()
        conf.closed_loop = True
        return WalkController(conf, num_envs=N, device="cuda:0"), None
    return walker(op3_walking_conf(RobotConfig()), N)


def throughput(kind, window=4000, windows=4, preroll=600):
    """Two identically built controllers, readouts off in one and on in the other, advanced over the SAME steps of the
    episode: each timed window of `window` steps runs on both, one after the other (the order alternates), so both modes
    time the same stretch of the gait.  A window is about a second of GPU time.  Also checks that the two stay
    bit-identical (the readouts do not change the state)."""
    pair = dict(off=controller(kind), on=controller(kind))
    pair["on"][0].enable_sim_readouts()

    def run(mode, k):
        wc, sched = pair[mode]
        with torch.cuda.stream(wc.tick_stream if sched is not None else torch.cuda.current_stream()):
            for _ in range(k):
                if sched is None:
                    wc.step()
                else:
                    wc.step_pipelined(walk=(sched, wc.t))
            wc.sync_sim()

    for mode in pair:
        run(mode, preroll)
    torch.cuda.synchronize()
    res = dict(off=[], on=[])
    for w in range(windows):
        for mode in (("off", "on") if w % 2 == 0 else ("on", "off")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(mode, window)
            torch.cuda.synchronize()
            res[mode].append(N * window / (time.perf_counter() - t0))
    a, b = pair["off"][0], pair["on"][0]
    identical = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("q", "v", "tau", "qpos", "qvel", "ncon", "con_pairs", "info"))
    ratio = [y / x - 1 for x, y in zip(res["off"], res["on"])]
    med = {k: float(np.median(v)) for k, v in res.items()}
    what = "closed-loop standing, step() back to back (tick + sim)" if kind == "standing" else \
        "open-loop walking, step_pipelined() with the walking update on tick_stream (bench.py's loop)"
    return dict(workload=what, envs=N, preroll_steps=preroll, window_steps=window, windows=windows,
                env_steps_per_s_median=med, all=res, on_vs_off_per_window=ratio, on_vs_off_median=float(np.median(ratio)),
                same_state_at_the_end=identical)


def realised(kind, seconds):
    if kind == "standing":
        conf = RobotConfig()
        conf.closed_loop = True
        wc, sched = WalkController(conf, num_envs=N, device="cuda:0"), None
    else:
        wc, sched = walker(op3_closed_loop_walking_conf(RobotConfig()), N, touchdown=True)
    wc.enable_sim_readouts()
    dt = wc.conf.dt
    steps = round(seconds / dt)
    cop_d, f_d, fz_sim, fz_tsid, n_cop = [], [], [], [], 0
    for i in range(steps):
        if sched is not None:
            sched.apply(wc, i * dt)
        wc.step()
        if i < steps // 4:      # (after the start-up transient)
            continue
        ok = wc.done == 0
        planned = wc.get_cop()
        real = wc.sim_cop()
        both = ok & torch.isfinite(planned[:, 0]) & torch.isfinite(real[:, 0])
        if bool(both.any()):
            cop_d.append((real[both, :2] - planned[both, :2]).norm(dim=1).double().cpu())
            n_cop += int(both.sum())
        # TSID's planned force per sole: the four corner forces of its Contact6d summed (f = LF 12 then RF 12)
        fp = wc.f.reshape(N, 2, 4, 3).sum(2)
        act = wc.contact_active.bool() & ok[:, None]
        if bool(act.any()):
            f_d.append((wc.foot_force - fp)[act].norm(dim=1).double().cpu())
            fz_sim.append(wc.foot_force[:, :, 2][act].double().cpu())
            fz_tsid.append(fp[:, :, 2][act].double().cpu())
    torch.cuda.synchronize()
    q = lambda v, p: round(float(np.quantile(torch.cat(v).numpy(), p)), 6) if v else None
    return dict(workload=f"closed-loop {kind}", envs=N, seconds=seconds, dt=dt, envs_done_at_the_end=int((wc.done != 0).sum()),
                cop_distance_m=dict(samples=n_cop, median=q(cop_d, 0.5), p95=q(cop_d, 0.95), max=q(cop_d, 1.0)),
                sole_force_difference_N=dict(median=q(f_d, 0.5), p95=q(f_d, 0.95), max=q(f_d, 1.0)),
                sole_fz_sim_N=dict(median=q(fz_sim, 0.5), p5=q(fz_sim, 0.05), p95=q(fz_sim, 0.95)),
                sole_fz_tsid_N=dict(median=q(fz_tsid, 0.5), p5=q(fz_tsid, 0.05), p95=q(fz_tsid, 0.95)))


if __name__ == "__main__":
    out = dict(device=torch.cuda.get_device_name(0), dtype="f64",
               cost=dict(standing=throughput("standing"), walking=throughput("walking")))
    if not COST_ONLY:
        out["realised_vs_planned"] = dict(standing=realised("standing", 2.0), walking=realised("walking", 4.0))
    text = json.dumps(out, indent=1)
    print(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
