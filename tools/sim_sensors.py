"""Site sensors of the sim stage (WalkController.enable_sensors; tsidb_set_sensors = mj_data.sensordata): what they cost.
Env-steps/s with the sensors off and on, measured as tools/sim_readouts.py measures the readouts: two identically built
controllers stepped over the same steps of the episode, timed windows of ~1 s alternating between them, closed-loop standing
(step() back to back) and open-loop walking, the headline workload (bench.py's loop: step_pipelined() with the walking
reference update in the tick, on WalkController.tick_stream); both controllers' states must be bit-identical at the end.
    python tools/sim_sensors.py [envs] [out.json] [sites]     (on an MI355X; default 4096 envs, profiles/sim_sensors.json,
                                                               sites = imu,lf_imu,rf_imu)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tsid_control_amd import RobotConfig, WalkController  # noqa: E402
from tsid_control_amd.walk_planner import WalkSchedule, op3_walking_conf, op3_walking_posture  # noqa: E402

ARGS = sys.argv[1:]
N = int(ARGS[0]) if len(ARGS) > 0 else 4096
OUT = ARGS[1] if len(ARGS) > 1 else "profiles/sim_sensors.json"
SITES = ARGS[2].split(",") if len(ARGS) > 2 else ["imu", "lf_imu", "rf_imu"]


def controller(kind):
    if kind == "standing":
        conf = RobotConfig()
        conf.closed_loop = True
        return WalkController(conf, num_envs=N, device="cuda:0"), None
    conf = op3_walking_conf(RobotConfig())
    wc = WalkController(conf, num_envs=N, device="cuda:0")
    wc.posture_ref += torch.as_tensor(op3_walking_posture(), device=wc.device).to(wc.dtype)
    lf, rf = wc.frames[0, 0, 9:11].cpu().numpy(), wc.frames[0, 1, 9:11].cpu().numpy()
    sched = WalkSchedule.from_demo_paths(N, conf, wc.device, wc.dtype, seed=1, q0_feet=(lf, rf),
                                         com0=wc.com_ref[0, :3].cpu().numpy(), foot_press=0.0, t_start=1.0)
    return wc, sched


def throughput(kind, window=4000, windows=4, preroll=600):
    pair = dict(off=controller(kind), on=controller(kind))
    pair["on"][0].enable_sensors(SITES)

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
    acc = b.accelerometer.double()
    return dict(workload=what, envs=N, sites=SITES, preroll_steps=preroll, window_steps=window, windows=windows,
                env_steps_per_s_median=med, all=res, on_vs_off_per_window=ratio, on_vs_off_median=float(np.median(ratio)),
                same_state_at_the_end=identical, accelerometer_norm_median=float(acc.norm(dim=2).median()))


if __name__ == "__main__":
    out = dict(device=torch.cuda.get_device_name(0), dtype="f64",
               cost=dict(standing=throughput("standing"), walking=throughput("walking")))
    text = json.dumps(out, indent=1)
    print(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
