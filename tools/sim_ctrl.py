"""Direct actuator control of the sim stage (WalkController.set_ctrl; tsidb_set_ctrl = mj_data.ctrl): what it costs.
(1) Env-steps/s with no ctrl buffer and with one registered (residual mode, all zero: the same trajectory), measured as
tools/sim_sensors.py measures the sensors: two identically built controllers stepped over the same steps of the episode, timed
windows alternating between them, closed-loop standing (step() back to back) and open-loop walking, the headline workload
(bench.py's loop: step_pipelined() with the walking reference update in the tick, on WalkController.tick_stream); both
controllers' states must be bit-identical at the end.
(2) sim_steps(8) - eight sim steps in one launch (tsidb_sim_ctrl) - against eight sim_step(teleport=False) launches, position
mode holding the standing pose, at 512 and 4096 envs.
    python tools/sim_ctrl.py [envs] [out.json]     (on an MI355X; default 4096 envs, profiles/sim_ctrl.json)"""
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
OUT = ARGS[1] if len(ARGS) > 1 else "profiles/sim_ctrl.json"


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
    on = pair["on"][0]
    on.set_ctrl(torch.zeros(N, on.NA, dtype=on.dtype, device=on.device), "residual")

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
    return dict(workload=what, envs=N, mode="residual, all-zero buffer", preroll_steps=preroll, window_steps=window, windows=windows,
                env_steps_per_s_median=med, all=res, on_vs_off_per_window=ratio, on_vs_off_median=float(np.median(ratio)),
                same_state_at_the_end=identical)


def multi_step(n, rounds=300, windows=4, preroll=100):
    """sim-steps/s of sim_steps(8) against 8 x sim_step(teleport=False): two controllers, position mode holding the standing
    pose (the robots stay on their feet: the same contact work throughout), alternating timed windows"""
    def one():
        wc = WalkController(RobotConfig(), num_envs=n, device="cuda:0")
        wc.set_ctrl(wc.ctrl_from_q(wc.q).contiguous(), "position")
        wc.qpos[:, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=wc.dtype, device=wc.device)   # (wxyz: no teleport writes it here)
        return wc
    pair = dict(single=one(), batched=one())

    def run(mode, k):
        wc = pair[mode]
        for _ in range(k):
            if mode == "single":
                for _ in range(8):
                    wc.sim_step(teleport=False)
            else:
                wc.sim_steps(8)

    for mode in pair:
        run(mode, preroll)
    torch.cuda.synchronize()
    res = dict(single=[], batched=[])
    for w in range(windows):
        for mode in (("single", "batched") if w % 2 == 0 else ("batched", "single")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(mode, rounds)
            torch.cuda.synchronize()
            res[mode].append(n * 8 * rounds / (time.perf_counter() - t0))
    a, b = pair["single"], pair["batched"]
    identical = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("qpos", "qvel", "ncon", "con_pairs", "info"))
    ratio = [y / x - 1 for x, y in zip(res["single"], res["batched"])]
    return dict(envs=n, sim_waves="library default (2 up to 512 envs, else 1)", rounds_of_8_steps_per_window=rounds, windows=windows,
                env_sim_steps_per_s_median={k: float(np.median(v)) for k, v in res.items()}, all=res,
                batched_vs_single_per_window=ratio, batched_vs_single_median=float(np.median(ratio)),
                same_state_at_the_end=identical, ncon_min=int(a.ncon.min()), standing_height=float(a.qpos[:, 2].min()))


if __name__ == "__main__":
    out = dict(device=torch.cuda.get_device_name(0), dtype="f64",
               cost=dict(standing=throughput("standing"), walking=throughput("walking")),
               sim_steps_8_vs_8_launches={str(n): multi_step(n) for n in (512, 4096)})
    text = json.dumps(out, indent=1)
    print(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
