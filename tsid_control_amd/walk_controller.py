"""WalkController - batched, MI355X-resident counterpart of the reference's ctrl/WalkController.py.

Same constructor argument (a RobotConfig), same attribute and method names
(ctrl/WalkController.py:11-295), but every quantity carries a leading env axis and lives in a
torch-ROCm tensor that the HIP kernels update in place through the C-ABI (include/tsidb.h).
`reset()` and `step()` are new: they encapsulate WalkController.py:22-26,72-79 + main.py:57-64 and
main.py:119-129,192-195 respectively (the reference writes that loop inline).

The task stack (what the reference builds with tsid calls at WalkController.py:54-187) is fixed
inside the kernels: 2x Contact6d (hard), 2x TaskSE3Equality, TaskComEquality, TaskJointPosture,
TaskActuationBounds, TaskJointBounds, SolverHQuadProgFast.  The `formulation`, `solver`, `robot`
objects of the reference have no counterpart - their work happens inside `step()`.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._policy_util import ptr as _ptr
from .conf import RobotConfig
from .model import ModelBlob
from .params import P_COUNT, pack_params
from .sim_pipeline import SimPipeline, StreamTable, streams_overlap

MAXCON = 32


class TrajectorySample:
    """Minimal stand-in for tsid.TrajectorySample for SE3 tasks: pos [N,12] (p, R column-major),
    vel [N,6], acc [N,6] (WalkController.py:195-196 passes such samples to setReference)."""

    def __init__(self, pos, vel=None, acc=None):
        self.pos = pos
        self.vel = vel if vel is not None else torch.zeros(pos.shape[0], 6, dtype=pos.dtype, device=pos.device)
        self.acc = acc if acc is not None else torch.zeros(pos.shape[0], 6, dtype=pos.dtype, device=pos.device)


class WalkController:
    def __init__(self, conf: RobotConfig = None, num_envs: int = None, device=None):
        self.conf = conf = conf if conf is not None else RobotConfig()
        self.num_envs = N = int(num_envs if num_envs is not None else getattr(conf, "num_envs", 1))
        self.device = torch.device(device if device is not None else getattr(conf, "device", "cuda"))
        if self.device.type != "cuda":
            raise _lib.TsidbError("WalkController needs a ROCm device: the hot path has no CPU implementation")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dt_name = getattr(conf, "dtype", "f64")
        self.dtype = {"f64": torch.float64, "f32": torch.float32}[dt_name]
        self.model = ModelBlob(getattr(conf, "model_blob", None))
        self.params = pack_params(conf, self.model.effort_limit, self.model.velocity_limit)
        # one library per robot: pick the build whose dimensions are the blob's (libtsidb.so = v1, libtsidb_v0.so = robot/v0)
        self._L = L = _lib.load_for(self.model["model_dims"])
        NJ_, NQ, NV, NA, self.NB, self.has_sim = _lib.dims(L)
        NOBS, NROW = NQ + NV + 12, NQ + NV + 14
        self.NQ, self.NV, self.NA, self.NOBS, self.NROW = NQ, NV, NA, NOBS, NROW
        self._h = C.c_void_p()
        self._pipe = None                        # the SimPipeline of step_pipelined(), made on first use
        self._streams = StreamTable(self.device)   # tick_stream and its sim stream
        self._geom_body = None
        raw = self.model.raw
        self._check(L.tsidb_create(raw, len(raw), self.params.ctypes.data_as(C.c_void_p), P_COUNT, N, self.device.index,
                                   0 if dt_name == "f64" else 1, C.byref(self._h)), "tsidb_create")

        z = lambda *s, dt=self.dtype: torch.zeros(*s, dtype=dt, device=self.device)
        # TSID state (WalkController.py:23-24) and sim state (main.py:51,64)
        self.q, self.v = z(N, NQ), z(N, NV)
        self.qpos, self.qvel, self.qacc_warmstart = z(N, NQ), z(N, NV), z(N, NV)
        # task references
        self.com_ref, self.posture_ref = z(N, 9), z(N, NA)
        self.foot_ref, self.contact_ref, self.cop_frames = z(N, 2, 24), z(N, 2, 12), z(N, 2, 12)
        self.contact_active = torch.ones(N, 2, dtype=torch.uint8, device=self.device)
        # outputs
        self.tau, self.dv, self.f = z(N, NA), z(N, NV), z(N, 24)
        self.status = z(N, dt=torch.int32)
        # one contiguous row per env = obs[65] + reward + done: what the all-gather sends
        self.rows = z(N, NROW)
        self.obs, self.reward, self.done = self.rows[:, :NOBS], self.rows[:, NOBS], self.rows[:, NOBS + 1]
        self.gather_width = NROW
        self.frames = z(N, 2, 12)
        self.ncon, self.con_pairs = z(N, dt=torch.int32), z(N, MAXCON, dt=torch.int32)
        self.info = z(N, 4, dt=torch.int32)
        self.env_params = None
        self.terrain = None
        self.xfrc = None   # external body wrenches [N, NB, 6] (set_xfrc / apply_push); None = none registered
        self.ctrl = None   # direct actuator control [N, NA] (set_ctrl); None = none registered
        self.ctrl_mode = None
        self._ctrl_qidx = None
        self._readouts = None   # sim-stage readout buffers (enable_sim_readouts); None = none registered
        self.con_force = self.con_frame = self.con_pos = self.con_dist = self.actuator_force = self.foot_force = self.foot_cop = None
        self.sensordata = None   # site sensors [N, S, 24] (enable_sensors); None = none registered
        self.framepos = self.framequat = self.framelinvel = self.frameangvel = self.velocimeter = self.gyro = self.accelerometer = None
        self._call("tsidb_set_refs", _ptr(self.com_ref), _ptr(self.posture_ref), _ptr(self.foot_ref), _ptr(self.contact_ref),
                   _ptr(self.contact_active), _ptr(self.cop_frames))
        sw = int(getattr(conf, "sim_waves", 0))   # 0 = the library's choice (2 wavefronts per env up to 512 envs, else 1)
        if sw:
            self._call("tsidb_set_option", _lib.OPT_SIM_WAVES, sw)
        fe = int(getattr(conf, "qp_fast_equalities", -1))   # -1 = the library's default (on)
        if fe >= 0:
            self._call("tsidb_set_option", _lib.OPT_QP_FAST_EQ, fe)
        self.cop_ref = z(N, 3)   # reference of the CoP force task (legacy/biped.py:79-80; conf.w_cop)
        self._call("tsidb_set_cop_ref", _ptr(self.cop_ref))

        # WalkController.py:168-169,179-180
        self.tau_max = conf.tau_max_scaling * self.model.effort_limit
        self.tau_min = -self.tau_max
        self.v_max = conf.v_max_scaling * self.model.velocity_limit
        self.v_min = -self.v_max
        self.LF_frame, self.RF_frame = 0, 1
        self.posture_bias = None
        self.t = 0.0
        b = int(getattr(conf, "pipeline_sim_batch", 0))
        # 0 = auto: small batches are latency bound, there the barrier packets of the per-step cross-stream handshake are
        # 15-20 % of a step (measured: 512 envs +7 %, 1024 +5 %, 2048 and up nothing / noise)
        self.sim_batch = min(8, b) if b > 0 else (8 if self.num_envs <= 1024 else 1)   # step_pipelined(): sim stages enqueued this many at a time (one launch: tsidb_sim_batch)
        self.reset()
        self.q0 = self.q.clone()  # WalkController.py:23 (after the z shift of :74, which aliases q0)

    def __del__(self):
        try:
            if self._h:
                self._pipe = None    # (its reference to the sim stream's wrapper is ours, not a caller's)
                self._streams.close(self._call)
                self._L.tsidb_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        _lib.check(self._L, self._h, rc, what)

    def _call(self, name, *args):
        """The one path into the library: self._L.<name>(self._h, *args) with self.device current; raises TsidbError with
        the library's message when the call fails."""
        with torch.cuda.device(self.device):
            rc = getattr(self._L, name)(self._h, *args)
        if rc:
            self._check(rc, name)

    def _buffer(self, method, arg, shape, t=None):
        """A caller's tensor to use in place - it must be contiguous, of `shape` and self.dtype, on self.device - or a new
        zero tensor if t is None."""
        if t is None:
            return torch.zeros(*shape, dtype=self.dtype, device=self.device)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != self.dtype or t.device != self.device \
                or not t.is_contiguous():
            what = (tuple(t.shape), t.dtype, t.device, t.is_contiguous()) if isinstance(t, torch.Tensor) else type(t)
            raise _lib.TsidbError(f"{method}: {arg} must be a contiguous {shape} {self.dtype} tensor on {self.device}, got {what}")
        return t

    def _written(self, sched=None):
        """Every tensor a tick or a sim step writes, for what is registered now (with a schedule: its touch-down latch too):
        what capture_steps() rewinds after its warm-up and a captured graph keeps alive.  A new optional buffer goes HERE."""
        yield from (self.q, self.v, self.qpos, self.qvel, self.qacc_warmstart, self.com_ref, self.posture_ref, self.foot_ref,
                    self.contact_ref, self.contact_active, self.frames, self.rows, self.tau, self.dv, self.f, self.status, self.ncon,
                    self.con_pairs, self.info, self.cop_ref)
        if self._readouts is not None:
            yield from self._readouts.values()
        if self.sensordata is not None:
            yield self.sensordata
        if sched is not None and sched.td_latch is not None:
            yield sched.td_latch

    @property
    def contactLF_active(self):
        return self.contact_active[:, 0].bool()

    @property
    def contactRF_active(self):
        return self.contact_active[:, 1].bool()

    def set_params(self):
        """Re-read self.conf (edited RobotConfig values) into the device-side constants."""
        self.sync_sim()  # sim stages step_pipelined() has not launched yet belong to the OLD constants: run them first
        self.params = pack_params(self.conf, self.model.effort_limit, self.model.velocity_limit)
        self._call("tsidb_set_params", self.params.ctypes.data_as(C.c_void_p), P_COUNT)

    def set_env_params(self, mass_scale=None, friction=None, floor_normal=None, floor_offset=None, terrain=None):
        """Per-env randomisation of the sim stage (BASELINE config 5; no reference counterpart): any
        of mass_scale [N], friction [N] (floor contacts), floor_normal [N,3] (normalised here), floor_offset [N],
        terrain = dict(direction [N,2], phase [N], step_length [N] or float, heights [N,16]): a stepped floor -
        the surface is raised along its normal by heights[cell & 15], cell = floor((direction . x_world_xy - phase)
        / step_length); terrain = "flat" registers the table of a level floor (zeros, 1 / step_length = 1), for a caller or a
        kernel (PolicyEnv(terrain=...)) to rewrite self.terrain in place.  Calling with no argument restores the nominal model."""
        self.sync_sim()  # a sim stage left in flight by step_pipelined() may still read the old table
        N = self.num_envs
        if mass_scale is None and friction is None and floor_normal is None and floor_offset is None:
            self.env_params = None
        else:
            ep = torch.zeros(N, 8, dtype=self.dtype, device=self.device)
            ep[:, 0], ep[:, 1], ep[:, 4] = 1.0, 1.0, 1.0
            if mass_scale is not None:
                ep[:, 0] = torch.as_tensor(mass_scale, dtype=self.dtype, device=self.device)
            if friction is not None:
                ep[:, 1] = torch.as_tensor(friction, dtype=self.dtype, device=self.device)
            if floor_normal is not None:
                nrm = torch.as_tensor(floor_normal, dtype=self.dtype, device=self.device).reshape(N, 3)
                ep[:, 2:5] = nrm / nrm.norm(dim=1, keepdim=True)
            if floor_offset is not None:
                ep[:, 5] = torch.as_tensor(floor_offset, dtype=self.dtype, device=self.device)
            self.env_params = ep
        if terrain is None:
            self.terrain = None
        elif isinstance(terrain, str):
            if terrain != "flat":
                raise _lib.TsidbError(f"set_env_params: terrain must be a dict, 'flat' or None, got {terrain!r}")
            self.terrain = torch.zeros(N, 20, dtype=self.dtype, device=self.device)
            self.terrain[:, 3] = 1.0
        else:
            tr = torch.zeros(N, 20, dtype=torch.float64)
            d = torch.as_tensor(terrain["direction"], dtype=torch.float64).reshape(N, 2)
            tr[:, 0:2] = d / d.norm(dim=1, keepdim=True)
            tr[:, 2] = torch.as_tensor(terrain.get("phase", 0.0), dtype=torch.float64)
            tr[:, 3] = 1.0 / torch.as_tensor(terrain["step_length"], dtype=torch.float64)
            tr[:, 4:] = torch.as_tensor(terrain["heights"], dtype=torch.float64).reshape(N, 16)
            self.terrain = tr.to(self.device, self.dtype).contiguous()
        self._call("tsidb_set_env_params", _ptr(self.env_params), _ptr(self.terrain))

    # ------------------------------------------------------------------ external wrenches (push recovery)
    def set_xfrc(self, t=None):
        """Register t [N, NB, 6] (self.dtype, on self.device, contiguous) as the sim stage's external body wrenches -
        MuJoCo's mj_data.xfrc_applied[1:] (include/tsidb.h tsidb_set_xfrc): per sim body (the blob's order, body 0 = the
        torso) force (3) then torque (3), world frame, at the body's centre of mass; read by every sim step until changed.
        The tensor is used in place, not copied: self.xfrc is it.  None unregisters (no external wrenches).
        A caller that writes self.xfrc in place while step_pipelined() / capture_steps() is in use must call sync_sim()
        first, as the methods here do: a sim stage left unlaunched would otherwise read the new values."""
        self.sync_sim()   # sim stages step_pipelined() has not launched yet belong to the old wrenches
        if t is not None:
            self._buffer("set_xfrc", "t", (self.num_envs, self.NB, 6), t)
        self._call("tsidb_set_xfrc", _ptr(t))
        self.xfrc = t

    def _xfrc_rows(self, env_ids):
        if self.xfrc is None:
            self.set_xfrc(torch.zeros(self.num_envs, self.NB, 6, dtype=self.dtype, device=self.device))
        if env_ids is None:
            return slice(None)
        if isinstance(env_ids, torch.Tensor):
            return env_ids.to(self.device).long().reshape(-1)
        return torch.as_tensor(np.asarray(env_ids, dtype=np.int64), device=self.device).reshape(-1)

    def apply_push(self, force, torque=None, body=0, env_ids=None):
        """Set the external wrench on sim body `body` (0 = torso; body_masses() lists the others) of the envs env_ids
        (None = all): force [3] or [n, 3], torque likewise (None = 0), world frame, at the body's centre of mass.  It acts on
        every sim step until changed (clear_pushes()) or the env is reset.  Registers a zero buffer on first use."""
        self.sync_sim()
        rows = self._xfrc_rows(env_ids)
        w = torch.zeros(6, dtype=self.dtype, device=self.device)
        f = torch.as_tensor(force, dtype=self.dtype, device=self.device)
        tq = torch.zeros(3, dtype=self.dtype, device=self.device) if torque is None else \
            torch.as_tensor(torque, dtype=self.dtype, device=self.device)
        if f.dim() == 1 and tq.dim() == 1:
            w[:3], w[3:] = f, tq
        else:
            w = torch.cat(torch.broadcast_tensors(f.reshape(-1, 3), tq.reshape(-1, 3)), dim=1)
        self.xfrc[rows, int(body)] = w

    def clear_pushes(self, env_ids=None):
        """Zero every external wrench of the envs env_ids (None = all)."""
        self.sync_sim()
        if self.xfrc is None:
            return
        self.xfrc[self._xfrc_rows(env_ids)] = 0

    # ------------------------------------------------------------------ direct actuator control (policy-driven stepping)
    def set_ctrl(self, t=None, mode="position"):
        """Register t [N, NA] (self.dtype, on self.device, contiguous) as the sim stage's actuator controls - MuJoCo's
        mj_data.ctrl (include/tsidb.h tsidb_set_ctrl) - in the MJCF actuator order, the order of self.actuator_force
        (ctrl_from_q / ctrl_from_tau permute TSID-ordered values into it); read by every sim step until changed.
        mode: "position" = joint targets [rad] for the model's position servos (replaces the targets taken from q, and tau in
        the closed loop); "motor" = motor torques [N m], unclamped (replaces the servos, or tau); "residual" = an offset to
        what the TSID stage supplies: to the joint targets [rad] in the open loop, to tau [N m] in the closed loop.  The base
        teleport of the open loop stays; the closed-loop tick still runs and writes self.tau.
        The tensor is used in place, not copied: self.ctrl is it.  None unregisters (TSID drives the joints again).
        reset() / reset_done() zero the rows of the envs they reset.
        A caller that writes self.ctrl in place while step_pipelined() / capture_steps() is in use must call sync_sim()
        first, as the methods here do: a sim stage left unlaunched would otherwise read the new values."""
        self.sync_sim()   # sim stages step_pipelined() has not launched yet belong to the old controls
        if t is None:
            self._call("tsidb_set_ctrl", None, _lib.CTRL_OFF)
            self.ctrl = self.ctrl_mode = None
            return
        if mode not in _lib.CTRL_MODES:
            raise _lib.TsidbError(f"set_ctrl: mode must be one of {sorted(_lib.CTRL_MODES)}, got {mode!r}")
        self._buffer("set_ctrl", "t", (self.num_envs, self.NA), t)
        self._call("tsidb_set_ctrl", _ptr(t), _lib.CTRL_MODES[mode])
        self.ctrl, self.ctrl_mode = t, mode

    def _ctrl_index(self, device):
        if self._ctrl_qidx is None or self._ctrl_qidx.device != device:
            self._ctrl_qidx = torch.as_tensor(np.asarray(self.model["mj_ctrl_qidx"], dtype=np.int64), device=device)
        return self._ctrl_qidx

    def ctrl_from_q(self, q):
        """[.., NA] joint positions in the actuator (ctrl) order from a TSID q [.., NQ]: q[..., mj_ctrl_qidx]."""
        return q[..., self._ctrl_index(q.device)]

    def ctrl_from_tau(self, tau):
        """[.., NA] joint torques in the actuator (ctrl) order from a TSID tau [.., NA]: tau[..., mj_ctrl_qidx - 7]."""
        return tau[..., self._ctrl_index(tau.device) - 7]

    def sim_steps(self, n):
        """n sim steps driven by self.ctrl alone (set_ctrl first), no teleport: the controls are held over the steps
        (zero-order hold), up to 8 steps per launch (tsidb_sim_ctrl) - bit-identical to n sim_step(teleport=False) calls.
        Returns (qpos, qvel)."""
        self.sync_sim()
        n = int(n)
        while n > 0:
            b = min(n, _lib.MAX_SIM_BATCH)
            self._call("tsidb_sim_ctrl", b, _ptr(self.qpos), _ptr(self.qvel), _ptr(self.qacc_warmstart), None, _ptr(self.ncon),
                       _ptr(self.con_pairs), _ptr(self.info), self._stream())
            n -= b
        return self.qpos, self.qvel

    # ------------------------------------------------------------------ sim-stage readouts (contacts, forces)
    def enable_sim_readouts(self, con_force=None, con_frame=None, con_pos=None, actuator_force=None, foot_grf=None):
        """Register the sim stage's readouts (include/tsidb.h tsidb_set_sim_readouts): what a MuJoCo caller reads after
        mj_step as mj_data.contact, mj_contactForce and mj_data.actuator_force.  Every sim step of step(), sim_step(),
        step_pipelined() and capture_steps() then writes them; a pipelined caller reads them after sync_sim(), like qpos.
        Each argument is a tensor to use in place (self.dtype, on self.device, contiguous) or None to allocate one:
        con_force [N, 32, 6], con_frame [N, 32, 9], con_pos [N, 32, 4], actuator_force [N, NA], foot_grf [N, 2, 6].
        Exposed as self.con_force (normal, tangent 1, tangent 2, torsional, 0, 0 in the contact frame: the force geom1 - the
        floor for floor contacts - exerts on geom2), self.con_frame [N, 32, 3, 3] (rows normal, t1, t2), self.con_pos
        [N, 32, 3] (world), self.con_dist [N, 32], self.actuator_force [N, NA] (ctrl order), self.foot_force [N, 2, 3]
        (world) and self.foot_cop [N, 2, 3] (LF, RF).  Contact rows follow con_pairs; rows >= ncon are zero.  reset() does
        not touch them."""
        self.sync_sim()   # sim stages step_pipelined() has not launched yet must write the buffers they were launched with
        N = self.num_envs
        want = dict(con_force=(N, MAXCON, 6), con_frame=(N, MAXCON, 9), con_pos=(N, MAXCON, 4), actuator_force=(N, self.NA),
                    foot_grf=(N, 2, 6))
        given = dict(con_force=con_force, con_frame=con_frame, con_pos=con_pos, actuator_force=actuator_force, foot_grf=foot_grf)
        bufs = {k: self._buffer("enable_sim_readouts", k, shape, given[k]) for k, shape in want.items()}
        self._call("tsidb_set_sim_readouts", *(_ptr(bufs[k]) for k in want))
        self._readouts = bufs
        self.con_force, self.actuator_force = bufs["con_force"], bufs["actuator_force"]
        self.con_frame = bufs["con_frame"].view(N, MAXCON, 3, 3)
        self.con_pos, self.con_dist = bufs["con_pos"][:, :, :3], bufs["con_pos"][:, :, 3]
        self.foot_force, self.foot_cop = bufs["foot_grf"][:, :, :3], bufs["foot_grf"][:, :, 3:]

    def disable_sim_readouts(self):
        """Unregister the readouts: the sim stage runs its kernels without them again (bit-identical state)."""
        self.sync_sim()
        self._call("tsidb_set_sim_readouts", None, None, None, None, None)
        self._readouts = None
        self.con_force = self.con_frame = self.con_pos = self.con_dist = self.actuator_force = self.foot_force = self.foot_cop = None

    # ------------------------------------------------------------------ site sensors (IMU, frame readouts)
    SENSOR_COLUMNS = dict(framepos=(0, 3), framequat=(3, 7), framelinvel=(7, 10), frameangvel=(10, 13), velocimeter=(13, 16),
                          gyro=(16, 19), accelerometer=(19, 22))

    def _named_site(self, name):
        if name == "imu":          # the free joint's frame: root_site of robot/v0/robot.xml:62
            return 0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)
        if name in ("lf_imu", "rf_imu"):   # the sole bodies: sole frame -> TSID joint -> sim joint -> body, as foot_grf finds them
            fp, s2t = self.model["pin_frame_parent"], list(self.model["mj_sim2tsid"])
            return 1 + s2t.index(int(fp[0 if name == "lf_imu" else 1]) - 1), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)
        raise _lib.TsidbError(f"enable_sensors: unknown site name {name!r} (known: 'imu', 'lf_imu', 'rf_imu')")

    def enable_sensors(self, sites=None, out=None):
        """Register site sensors of the sim stage (include/tsidb.h tsidb_set_sensors): what a MuJoCo caller reads after
        mj_step as mj_data.sensordata.  sites = a list (1 .. 16 entries) of names or (body, pos [3], quat [4] wxyz) tuples in
        the body's own frame (sim body order, 0 = torso): "imu" is body 0 at the origin with identity orientation (the free
        joint's frame), "lf_imu" / "rf_imu" the two sole bodies' frames; default ["imu"].  out = a tensor to use in place
        ([N, S, 24], self.dtype, on self.device, contiguous) or None to allocate one.  Every sim step of step(), sim_step(),
        step_pipelined() and capture_steps() then writes the rows; a pipelined caller reads them after sync_sim(), like qpos.
        Exposed as self.sensordata [N, S, 24] and as views under MuJoCo's names: framepos, framelinvel, frameangvel (world
        frame), velocimeter, gyro, accelerometer (site frame) [N, S, 3] and framequat [N, S, 4] (wxyz).  As in mj_step the
        rows describe the positions and velocities the step STARTED from and the acceleration it solved for; the
        accelerometer reads R^T (0, 0, g) at rest and 0 in free fall.  reset() does not touch them."""
        self.sync_sim()   # sim stages step_pipelined() has not launched yet must write the buffer they were launched with
        sites = ["imu"] if sites is None else list(sites)
        S, N = len(sites), self.num_envs
        if not 1 <= S <= 16:
            raise _lib.TsidbError(f"enable_sensors: need 1 .. 16 sites, got {S}")
        body, pos, quat = np.zeros(S, np.int32), np.zeros((S, 3)), np.zeros((S, 4))
        for i, st in enumerate(sites):
            b, p, q = self._named_site(st) if isinstance(st, str) else st
            body[i], pos[i], quat[i] = int(b), np.asarray(p, dtype=np.float64).reshape(3), np.asarray(q, dtype=np.float64).reshape(4)
        out = self._buffer("enable_sensors", "out", (N, S, 24), out)
        vp = C.c_void_p
        self._call("tsidb_set_sensors", S, body.ctypes.data_as(vp), pos.ctypes.data_as(vp), quat.ctypes.data_as(vp), _ptr(out))
        self.sensordata = out
        for k, (a, b) in self.SENSOR_COLUMNS.items():
            setattr(self, k, out[:, :, a:b])

    def disable_sensors(self):
        """Unregister the site sensors: the sim stage runs its kernels without them again (bit-identical state)."""
        self.sync_sim()
        self._call("tsidb_set_sensors", 0, None, None, None, None)
        self.sensordata = None
        for k in self.SENSOR_COLUMNS:
            setattr(self, k, None)

    def sim_cop(self):
        """[N, 3] centre of pressure the sim realised on the floor: both soles' CoPs weighted by their normal force (the floor
        normal of set_env_params, else +z) - the counterpart of get_cop().  NaN where neither sole carries a normal force."""
        if self._readouts is None:
            raise _lib.TsidbError("sim_cop needs enable_sim_readouts()")
        nrm = self.env_params[:, 2:5] if self.env_params is not None else \
            torch.tensor([0.0, 0.0, 1.0], dtype=self.dtype, device=self.device).expand(self.num_envs, 3)
        w = (self.foot_force * nrm[:, None, :]).sum(-1)          # [N, 2] normal force per sole
        tot = w.sum(1, keepdim=True)
        cop = (w[:, :, None] * self.foot_cop).sum(1) / tot
        return torch.where(tot > 0, cop, torch.full_like(cop, float("nan")))

    def contact_bodies(self):
        """[N, 32, 2] int32 (body1, body2) of each row of con_pairs: sim bodies (the blob's order, 0 = torso) of geom1 and
        geom2 (mj_data.contact.geom -> mj_geom_body); the floor is -1.  Rows >= ncon are (-1, -1)."""
        gb = self._geom_body
        if gb is None:
            gb = self._geom_body = torch.as_tensor(np.asarray(self.model["mj_geom_body"], dtype=np.int64), device=self.device)
        cp = self.con_pairs.long()
        live = cp >= 0
        g2 = torch.where(live, cp >> 16, torch.zeros_like(cp))
        hh = live & ((cp & 0x8000) != 0)                          # robot<->robot: the low bits carry geom1
        g1 = torch.where(hh, cp & 0x7fff, torch.zeros_like(cp))
        b2 = torch.where(live, gb[g2], torch.full_like(cp, -1))
        b1 = torch.where(hh, gb[g1], torch.full_like(cp, -1))
        return torch.stack([b1, b2], dim=-1).to(torch.int32)

    def body_masses(self):
        """[N, NB] mass of every sim body (the blob's mj_inertia[:, 0] times the env's mass scale, set_env_params): what a
        uniform acceleration field a needs as forces, F_b = m_b a.  v1 robot (robot.xml document order): torso 0, left
        foot 6, right foot 12, camera enclosure 20."""
        m = torch.as_tensor(self.model["mj_inertia"].reshape(self.NB, 10)[:, 0].copy(), dtype=self.dtype, device=self.device)
        scale = self.env_params[:, 0:1] if self.env_params is not None else torch.ones(self.num_envs, 1, dtype=self.dtype, device=self.device)
        return scale * m

    def randomize(self, seed=2, mass=(0.8, 1.2), friction=(0.4, 1.0), tilt_deg=5.0, step_height=0.01, step_length=(0.04, 0.12)):
        """BASELINE config 5 workload: body-mass scale U(mass), contact friction
        U(friction), floor = random plane through the origin tilted by at most tilt_deg, with terrain steps of
        step_height (1 cm): strips of width U(step_length) across a random horizontal direction, each strip raised
        by 0 or step_height at random (period 16 strips; the strip under the robot's start is level).
        step_height = 0 leaves the floor a plane."""
        g = torch.Generator().manual_seed(seed)
        N = self.num_envs
        u = lambda lo, hi: lo + (hi - lo) * torch.rand(N, generator=g, dtype=torch.float64)
        tilt = torch.deg2rad(u(0.0, tilt_deg))
        az = u(0.0, 2 * np.pi)
        nrm = torch.stack([torch.sin(tilt) * torch.cos(az), torch.sin(tilt) * torch.sin(az), torch.cos(tilt)], dim=1)
        terrain = None
        if step_height > 0:
            ang = u(0.0, 2 * np.pi)
            length = u(*step_length)
            heights = step_height * torch.randint(0, 2, (N, 16), generator=g).to(torch.float64)
            heights[:, 0] = 0.0
            heights[:, 15] = 0.0
            # cell 0 is centred on the world origin (where every env's robot starts): phase = -length / 2
            terrain = dict(direction=torch.stack([torch.cos(ang), torch.sin(ang)], dim=1), phase=-0.5 * length,
                           step_length=length, heights=heights)
        self.set_env_params(mass_scale=u(*mass), friction=u(*friction), floor_normal=nrm,
                            floor_offset=torch.zeros(N, dtype=torch.float64), terrain=terrain)

    # ------------------------------------------------------------------ reset / step
    def set_posture_bias(self, bias):
        """[NA] offsets every reset adds to the posture reference it captures (ctrl/WalkController.py:164-165 takes q0's
        joints; a walking workload keeps its knees bent: walk_planner.op3_walking_posture()).  Also applied to the
        current posture references; None removes it."""
        old = self.posture_bias
        new = None if bias is None else torch.as_tensor(np.asarray(bias), device=self.device).to(self.dtype).contiguous()
        if old is not None:
            self.posture_ref -= old
        if new is not None:
            self.posture_ref += new
        self.posture_bias = new
        self._call("tsidb_set_posture_bias", _ptr(new))

    def reset_done(self, sched=None, t=None, new_paths=True):
        """Episode lifecycle on the device: reset every env whose done flag (self.done, written by the last tick) is set -
        standing state, references, sim state - and, with a WalkSchedule.on_device schedule, rebuild its plan (a new path
        when new_paths) and restart its clock at time t (default self.t, the time of the next tick).  Nothing comes back
        to the host; envs that are not done are untouched."""
        self.sync_sim()
        self._call("tsidb_reset_done", _ptr(self.rows), self.NROW, _ptr(self.q), _ptr(self.v), _ptr(self.qpos), _ptr(self.qvel),
                   _ptr(self.qacc_warmstart), _ptr(self.frames), self._stream())
        if sched is not None:
            sched.plan(self, t=self.t if t is None else t, done_only=True, new_paths=new_paths)

    def reset(self, env_ids=None, sched=None, t=None, new_paths=False):
        """Standing state with the soles on z = 0 and all references re-captured
        (WalkController.py:22-26,72-79,81,122,151-152,164-165; main.py:57-64).  sched (a WalkSchedule.on_device
        schedule): the reset envs' plans are rebuilt on the device (new paths when new_paths) and their clocks restart at
        time t (default: self.t after the reset, i.e. 0 for a full reset)."""
        self.sync_sim()  # step_pipelined() may have left a sim stage running on the side stream
        ids = None
        n_ids = 0
        if env_ids is not None:
            ids = torch.as_tensor(env_ids, dtype=torch.int32, device=self.device).contiguous()
            n_ids = ids.numel()
            if n_ids == 0:
                return  # nothing to reset (the C entry point reads a NULL id list as "every env")
        self._call("tsidb_reset", _ptr(ids), n_ids, _ptr(self.q), _ptr(self.v), _ptr(self.qpos), _ptr(self.qvel),
                   _ptr(self.qacc_warmstart), self._stream())
        if env_ids is None:
            self.frames.copy_(self.cop_frames)
            self.t = 0.0
        else:
            self.frames[ids.long()] = self.cop_frames[ids.long()]
        if sched is not None:
            sched.plan(self, env_ids=ids, t=self.t if t is None else t, new_paths=new_paths)

    def step(self, n_substeps: int = 1):
        """One env step for every env: TSID tick (main.py:119-129) then, if conf.sim_enabled, base
        teleport + joint targets + sim step (main.py:192-195).  Returns (tau, q, v, status, obs);
        all are views of the controller's tensors, updated in place."""
        self.sync_sim()
        self._call("tsidb_step", _ptr(self.q), _ptr(self.v), _ptr(self.qpos), _ptr(self.qvel), _ptr(self.qacc_warmstart),
                   _ptr(self.tau), _ptr(self.dv), _ptr(self.f), _ptr(self.status), _ptr(self.rows), self.NROW, _ptr(self.frames),
                   _ptr(self.ncon), _ptr(self.con_pairs), _ptr(self.info), int(n_substeps), self._stream())
        self.t += n_substeps * self.conf.dt
        return self.tau, self.q, self.v, self.status, self.obs

    def step_pipelined(self, events=None, walk=None):
        """One env step with the sim stage left running on a second HIP stream, so that it overlaps with
        what the caller enqueues next on the current stream - normally the TSID tick of the NEXT step.  The reference
        couples the two stages one way (the sim never feeds back into TSID, main.py:119-129 vs :192-195), so sim(t) and
        tick(t+1) are independent; the TSID state is handed to the sim through a ring of snapshot slots the tick writes.
        walk = (schedule, t) runs that tick's WalkSchedule.apply inside the tick's launch (tsidb_tick_walk).
        tau, q, v, status, obs are valid on the current stream as after step(); the sim state (qpos, qvel,
        qacc_warmstart, ncon, con_pairs, info[:, 2:4], and the readouts of enable_sim_readouts()) is valid after sync_sim() ONLY: with conf.pipeline_sim_batch > 1
        (the default for up to 1024 envs is 8) the last few sim stages are not even launched until the batch is full, so a
        device / stream synchronize does not make the sim state current - sync_sim() launches them and makes the current
        stream wait.  Every entry point of this class that reads or rewrites sim-side data (step, sim_step, reset,
        reset_done, set_params, set_env_params, set_xfrc, apply_push, clear_pushes, set_ctrl, sim_steps, enable_sim_readouts, disable_sim_readouts, enable_sensors, disable_sensors,
        capture_steps, WalkSchedule.apply with touch-down feedback) calls it.
        `events` = four torch.cuda.Event recorded around the tick (current stream) and around the sim (sim stream), for
        timing."""
        if getattr(self.conf, "closed_loop", False) or not getattr(self.conf, "sim_enabled", True):
            raise _lib.TsidbError("step_pipelined needs the open-loop sim stage (closed loop: the tick reads the sim state)")
        cur = torch.cuda.current_stream(self.device)
        P = self._ensure_pipe()
        slot = P.next_slot(cur)                # (waits for the sim batch that read this slot 2 * sim_batch steps ago)
        if events:
            events[0].record(cur)
        # the tick writes the TSID state it ends on into the slot as well (two copy kernels less on this stream); walk =
        # (schedule, t): the walking reference update of this tick in the same launch
        self.tick(walk=walk, _snap=(P.q[slot], P.v[slot]))
        if events:
            events[1].record(cur)
        P.pending.append(slot)
        # conf.pipeline_sim_batch > 1 enqueues the sim stages that many at a time, as one launch (one cross-stream wait and one
        # record per batch instead of per step, no launch gaps; the sim state then lags the tick by up to that many steps
        # until sync_sim()).  Measured (DESIGN.md section 5 "Streams"): no gain from 2048 envs on; 512 / 1024 walkers +25-30 %
        # together with the fused tick launch (8 at a time, the default for up to 1024 envs).
        if len(P.pending) >= self.sim_batch or events:
            P.flush(cur, self._sim_batch, events)
        self.t += self.conf.dt
        return self.tau, self.q, self.v, self.status, self.obs

    def _streams_overlap(self, sa, sb):   # bench.py places its collective's stream with it
        return streams_overlap(self.device, sa, sb)

    @property
    def tick_stream(self):
        """The stream to run the pipelined loop on: `with torch.cuda.stream(wc.tick_stream): wc.step_pipelined(...)`.  For up
        to 512 envs it is restricted to one half of the CUs and the sim stream to the other (the two kernels slow each other
        down by a quarter when they share CU groups: +11-14 % env-steps/s at 256 / 512 envs); otherwise an ordinary stream.
        Optional - step_pipelined() works on any current stream; the sim stream is paired with this one only if the FIRST
        step_pipelined() runs on it."""
        return self._streams.get(_lib.ROLE_TICK, self._call)

    def _ensure_pipe(self):
        """the SimPipeline (sim_pipeline.py: the second stream and the ring of snapshot slots) of step_pipelined(); (re)built
        when missing or too small for the current sim batch"""
        need = min(16, max(4, 2 * self.sim_batch))
        if self._pipe is None or len(self._pipe.q) < need:
            self.sync_sim()                     # nothing may be pending in the ring that is replaced
            self._pipe = SimPipeline(self._streams.sim_stream_for(torch.cuda.current_stream(self.device)), self.q, self.v, need)
        return self._pipe

    def gather_rows(self, out=None):
        """[N, 67] = obs, reward, done of the last tick: the per-env row the multi-GPU all-gather carries."""
        if out is None:
            return self.rows
        out.copy_(self.rows)
        return out

    def capture_steps(self, n_steps: int, sched=None, sim_batch: int = None):
        """Capture n_steps pipelined env steps (walking reference update, TSID tick, sim step on the second stream)
        in ONE HIP graph and return it; graph.replay() then enqueues all of them with a single launch instead of
        ~8 host calls per step - what bounds small batches (512-1024 envs per GPU: the strong split of 4096 walkers
        over 4-8 GPUs).  The schedule's clock lives on the device (self.t_device, advanced inside the graph); results
        are bit-identical to the same number of step_pipelined() calls with the same number of sim steps per launch (float32:
        a different number of sim steps per launch agrees to rounding only, include/tsidb.h tsidb_sim_batch).  The sim state
        is valid after sync_sim().
        sim_batch = sim steps per launch INSIDE the graph (default: as in eager mode).  A graph ends with a join, so the
        sim batch still to run after the last tick runs alone; measured (512 envs): eager 6.64 M
        env-steps/s; 16 steps per graph 5.2 / 5.5 / 5.2 M with 1 / 2 / 8 sim steps per launch, 64 steps per graph 5.8 / 6.0 /
        6.4 M - replaying a graph never beats the eager pipeline here."""
        if getattr(self.conf, "closed_loop", False) or not getattr(self.conf, "sim_enabled", True):
            raise _lib.TsidbError("capture_steps uses the open-loop pipeline (step_pipelined)")
        dt = self.conf.dt
        self.sync_sim()   # the state saved below must include the sim stage a previous step_pipelined() left in flight
        P = self._ensure_pipe()   # (the ring sized for the eager batch: it is not rebuilt, and the graph's pointers stay valid, afterwards)
        batch_keep = self.sim_batch
        if sim_batch is not None:
            self.sim_batch = max(1, min(int(sim_batch), len(P.q) // 2))
        self.t_device = torch.full((1,), self.t, dtype=torch.float64, device=self.device)   # float64 whatever the path's dtype
        # warm up outside the capture (lazy kernel loads, cached contiguous tables), then rewind the state
        written = list(self._written(sched))
        saved = [t.clone() for t in written]
        t_keep = self.t
        if sched is not None:
            sched.apply(self, self.t, t_device=self.t_device)
        self.step_pipelined()
        self.t_device += dt
        self.sync_sim()
        torch.cuda.synchronize(self.device)
        for t, s in zip(written, saved):
            t.copy_(s)
        self.t = t_keep
        self.t_device.fill_(self.t)
        P.forget_events()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n_steps):
                self.step_pipelined(walk=(sched, 0.0, self.t_device) if sched is not None else None)
                self.t_device += dt
            self.sync_sim()                 # join the sim stream: the graph ends with every kernel done
        P.forget_events()
        self.sim_batch = batch_keep
        self.t = t_keep                     # the capture advanced the host clock without running anything

        outer = self

        class _Graph:
            steps = n_steps
            keep = (P.qring, P.vring, P.stream, self.xfrc, self.ctrl, *written)   # what the captured kernels point at

            def replay(self_inner):
                g.replay()
                for _ in range(n_steps):   # the same additions the device clock and step_pipelined() make
                    outer.t += dt

        return _Graph()

    def _sim_batch(self, slots):
        """the sim stages of several ticks in ONE launch (tsidb_sim_batch): each env steps len(slots) times, teleporting to
        the snapshot of its tick each time - no launch gaps between the steps"""
        B, P = len(slots), self._pipe
        if B == 1:
            self.sim_step(q_tsid=P.q[slots[0]], v_tsid=P.v[slots[0]], _from_pipe=True)
            return
        self._call("tsidb_sim_batch", B, _ptr(P.qring), _ptr(P.vring), (C.c_int32 * B)(*slots), _ptr(self.qpos), _ptr(self.qvel),
                   _ptr(self.qacc_warmstart), None, _ptr(self.ncon), _ptr(self.con_pairs), _ptr(self.info), self._stream())

    def sync_sim(self):
        """Make the current stream wait for the sim stages step_pipelined() left in flight (or not yet enqueued)."""
        if self._pipe is not None:
            self._pipe.join(torch.cuda.current_stream(self.device), self._sim_batch)

    def tick(self, walk=None, _snap=None):
        """TSID stage only (main.py:119-129).  walk = (schedule, t): that tick's walking reference update
        (WalkSchedule.apply(self, t)) runs in the same launch, ahead of the tick (tsidb_tick_walk) - same results."""
        if walk is None and _snap is None:
            self._call("tsidb_tick", _ptr(self.q), _ptr(self.v), _ptr(self.tau), _ptr(self.dv), _ptr(self.f), _ptr(self.status),
                       _ptr(self.rows), self.NROW, _ptr(self.frames), _ptr(self.info), self._stream())
            return self.tau, self.q, self.v, self.status, self.obs
        wa = walk[0].args(self, walk[1], *walk[2:]) if walk is not None else None
        qs, vs = _snap if _snap is not None else (None, None)
        self._call("tsidb_tick_walk", C.byref(wa) if wa is not None else None, _ptr(self.q), _ptr(self.v), _ptr(self.tau),
                   _ptr(self.dv), _ptr(self.f), _ptr(self.status), _ptr(self.rows), self.NROW, _ptr(self.frames), _ptr(self.info),
                   _ptr(qs), _ptr(vs), self._stream())
        return self.tau, self.q, self.v, self.status, self.obs

    def sim_step(self, teleport=True, q_tsid=None, v_tsid=None, _from_pipe=False):
        """Sim stage only (main.py:192-195); teleport=False steps the sim state on its own; q_tsid / v_tsid
        override the TSID state the base pose / joint targets (and, with reference_quirks=False, the base
        velocity) are taken from (snapshots of self.q / self.v when the sim stage runs on another stream
        than the tick)."""
        if not _from_pipe:
            self.sync_sim()
        src = q_tsid if q_tsid is not None else self.q
        srcv = v_tsid if v_tsid is not None else self.v
        self._call("tsidb_sim", _ptr(src) if teleport else None, _ptr(srcv) if teleport else None, _ptr(self.qpos), _ptr(self.qvel),
                   _ptr(self.qacc_warmstart), None, _ptr(self.ncon), _ptr(self.con_pairs), _ptr(self.info), self._stream())
        return self.qpos, self.qvel

    def rbd_terms(self, q=None, v=None):
        """Rigid-body terms of computeProblemData (main.py:119) for inspection/tests."""
        q = self.q if q is None else q
        v = self.v if v is None else v
        N = self.num_envs
        z = lambda *s: torch.zeros(*s, dtype=self.dtype, device=self.device)
        NV = self.NV
        out = dict(M=z(N, NV, NV), h=z(N, NV), Jcom=z(N, 3, NV), Jf=z(N, 2, 6, NV), oMf=z(N, 2, 12), com=z(N, 3))
        self._call("tsidb_rbd_terms", _ptr(q), _ptr(v), _ptr(out["M"]), _ptr(out["h"]), _ptr(out["Jcom"]), _ptr(out["Jf"]),
                   _ptr(out["oMf"]), _ptr(out["com"]), self._stream())
        return out

    # ------------------------------------------------------------------ reference method surface
    @staticmethod
    def _frames_to_se3vec(fr):
        """[.., 12] R row-major + p  ->  [.., 12] p + R column-major (tsid SE3ToVector)."""
        R = fr[..., :9].reshape(*fr.shape[:-1], 3, 3)
        return torch.cat([fr[..., 9:], R.transpose(-1, -2).reshape(*fr.shape[:-1], 9)], dim=-1)

    def _mask(self, flag):
        if isinstance(flag, torch.Tensor):
            return flag.to(self.device).bool().reshape(-1)
        return torch.full((self.num_envs,), bool(flag), dtype=torch.bool, device=self.device)

    def _sample24(self, s):
        if isinstance(s, torch.Tensor):
            return s.to(self.device, self.dtype).reshape(self.num_envs, 24)
        return torch.cat([s.pos, s.vel, s.acc], dim=-1).to(self.device, self.dtype).reshape(self.num_envs, 24)

    def update_tasks(self, sampleLF, sampleRF, contact_LF, contact_RF):
        """WalkController.py:189-209, batched: set both foot-task references, then switch contacts
        on the edges of the (per-env) contact flags."""
        self.foot_ref[:, 0] = self._sample24(sampleLF)
        self.foot_ref[:, 1] = self._sample24(sampleRF)
        cLF, cRF = self._mask(contact_LF), self._mask(contact_RF)
        aLF, aRF = self.contactLF_active, self.contactRF_active
        self.add_contact(left_foot=cLF & ~aLF, right_foot=cRF & ~aRF)
        self.remove_contact(left_foot=~cLF & aLF, right_foot=~cRF & aRF)

    def display(self, q):
        """WalkController.py:211-213: viewer hook; no viewer exists here."""
        return None

    def remove_contact(self, left_foot=True, right_foot=True):
        """WalkController.py:215-232 (as legacy/biped.py:168-189 makes it work): re-reference the foot
        task at the current placement, drop the rigid contact."""
        cur = self._frames_to_se3vec(self.frames)
        for f, flag in ((0, left_foot), (1, right_foot)):
            m = self._mask(flag) & self.contact_active[:, f].bool()
            ref = torch.cat([cur[:, f], torch.zeros(self.num_envs, 12, dtype=self.dtype, device=self.device)], dim=-1)
            self.foot_ref[:, f] = torch.where(m[:, None], ref, self.foot_ref[:, f])
            self.contact_active[:, f] = torch.where(m, torch.zeros_like(self.contact_active[:, f]), self.contact_active[:, f])

    def add_contact(self, left_foot=True, right_foot=True):
        """WalkController.py:234-253: re-reference the contact at the current placement, add it back."""
        cur = self._frames_to_se3vec(self.frames)
        for f, flag in ((0, left_foot), (1, right_foot)):
            m = self._mask(flag) & ~self.contact_active[:, f].bool()
            self.contact_ref[:, f] = torch.where(m[:, None], cur[:, f], self.contact_ref[:, f])
            self.contact_active[:, f] = torch.where(m, torch.ones_like(self.contact_active[:, f]), self.contact_active[:, f])

    def get_cop(self, sol=None):
        """WalkController.py:255-289: centre of pressure of the last tick's contact forces, [N,3];
        rows are NaN where the reference would return None (not both feet in contact)."""
        o = self.NQ + self.NV
        cop = self.obs[:, o + 3:o + 6].clone()
        both = self.contactLF_active & self.contactRF_active
        cop[~both] = float("nan")
        return cop

    def compute_capture_point(self, com=None, dcom=None, w=None):
        """legacy/biped.py:224-227, batched: cp = com + dcom / w with cp_z = 0; defaults to the last tick's
        CoM / CoM velocity (obs) and the LIPM frequency of the current CoM height."""
        com = self.obs[:, self.NQ + self.NV:self.NQ + self.NV + 3] if com is None else com
        if dcom is None:
            raise ValueError("dcom (CoM velocity [N,3]) is required: the observation vector carries positions only")
        if w is None:
            w = torch.sqrt(9.80665 / com[:, 2:3])
        cp = com + dcom / w
        cp[:, 2] = 0
        return cp

    def compute_support_polygon(self):
        """legacy/biped.py:229-234, batched: the two sole positions in the plane, [N, 2 (LF, RF), 2]."""
        return self.frames[:, :, 9:11].clone()

    def integrate_dv(self, q, v, dv, dt):
        """WalkController.py:291-295 for caller-held tensors: v updated in place, new q returned.
        (step() integrates inside the kernel; this exists for callers that drive the pieces.)"""
        v_mean = v + 0.5 * dt * dv
        v += dt * dv
        d = dt * v_mean
        w = d[:, 3:6]
        th = torch.linalg.norm(w, dim=-1, keepdim=True)
        th2 = th * th
        small = th < 1e-8
        ths = torch.where(small, torch.ones_like(th), th)
        b = torch.where(small, 0.5 - th2 / 24, (1 - torch.cos(ths)) / (ths * ths))
        c = torch.where(small, 1.0 / 6 - th2 / 120, (ths - torch.sin(ths)) / (ths ** 3))
        sh = torch.where(small, 0.5 - th2 / 48, torch.sin(0.5 * ths) / ths)
        ch = torch.cos(0.5 * th)
        wxv = torch.cross(w, d[:, :3], dim=-1)
        pd = d[:, :3] + b * wxv + c * torch.cross(w, wxv, dim=-1)
        x, y, z_, w_ = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
        R = torch.stack([1 - 2 * (y * y + z_ * z_), 2 * (x * y - w_ * z_), 2 * (x * z_ + w_ * y),
                         2 * (x * y + w_ * z_), 1 - 2 * (x * x + z_ * z_), 2 * (y * z_ - w_ * x),
                         2 * (x * z_ - w_ * y), 2 * (y * z_ + w_ * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
        qn = q.clone()
        qn[:, :3] = q[:, :3] + (R @ pd[:, :, None])[:, :, 0]
        dq = torch.cat([sh * w, ch], dim=-1)
        a = q[:, 3:7]
        r = torch.stack([
            a[:, 3] * dq[:, 0] + a[:, 0] * dq[:, 3] + a[:, 1] * dq[:, 2] - a[:, 2] * dq[:, 1],
            a[:, 3] * dq[:, 1] - a[:, 0] * dq[:, 2] + a[:, 1] * dq[:, 3] + a[:, 2] * dq[:, 0],
            a[:, 3] * dq[:, 2] + a[:, 0] * dq[:, 1] - a[:, 1] * dq[:, 0] + a[:, 2] * dq[:, 3],
            a[:, 3] * dq[:, 3] - a[:, 0] * dq[:, 0] - a[:, 1] * dq[:, 1] - a[:, 2] * dq[:, 2]], dim=-1)
        qn[:, 3:7] = r / torch.linalg.norm(r, dim=-1, keepdim=True)
        qn[:, 7:] = q[:, 7:] + d[:, 6:]
        return qn, v


def map_tsid_to_mujoco(q_tsid, model: ModelBlob = None):
    """main.py:11-44, batched: joint-angle targets in the sim's actuator order from a TSID q."""
    model = model or ModelBlob()
    idx = torch.as_tensor(np.asarray(model["mj_ctrl_qidx"]), dtype=torch.long, device=q_tsid.device)
    return q_tsid[..., idx]
