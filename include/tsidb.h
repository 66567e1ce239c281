/* tsidb.h - C-ABI of the MI355X-native batched TSID + contact-dynamics path (libtsidb.so).
 *
 * The reference (UW-RoboSoccer/tsid_control) has no FFI for this path: its boundary is the Python
 * call surface of main.py:119-129,192-195 against ctrl/WalkController.py and ctrl/conf.py.  Each
 * entry point below names the reference calls it stands for.  All state/output buffers are device
 * pointers owned by the caller (torch-ROCm tensors), env-major and contiguous, in the arithmetic
 * type chosen at create time (TSIDB_F64 = the reference's float64, TSIDB_F32); the library owns only
 * the handle (model constants).  Calls are asynchronous on the given HIP stream (hipStream_t passed
 * as void*).  Return 0 = OK, non-zero = library-level failure (message via tsidb_last_error);
 * a per-env QP failure is data in status[e] (tsid HQPStatus codes: 0 optimal, 1 infeasible,
 * 2 unbounded, 3 max-iter, 4 error), never a call failure - mirroring main.py:122-124 without
 * aborting the batch: that env's tau, dv and f are 0 for the tick, its TSID state is left as it was, done = 1.
 * A handle is not thread-safe; one handle per GPU.
 */
#ifndef TSIDB_H
#define TSIDB_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsidb_ctx *tsidb_handle;

enum { TSIDB_F64 = 0, TSIDB_F32 = 1 };
enum { TSIDB_NQ = 27, TSIDB_NV = 26, TSIDB_NA = 20, TSIDB_NOBS = 65, TSIDB_NROW = 67, TSIDB_MAXCON = 32 };

/* parameter vector (float64, host): RobotConfig values the reference hands to its task
 * constructors (ctrl/conf.py:21-72 via ctrl/WalkController.py:55-184) */
enum {
  TSIDB_P_DT = 0, TSIDB_P_MU, TSIDB_P_FMIN, TSIDB_P_FMAX, TSIDB_P_W_FORCEREF, TSIDB_P_KP_CONTACT,
  TSIDB_P_KD_CONTACT, TSIDB_P_W_FOOT, TSIDB_P_KP_FOOT, TSIDB_P_KD_FOOT, TSIDB_P_W_COM, TSIDB_P_KP_COM,
  TSIDB_P_KD_COM, TSIDB_P_W_POSTURE, TSIDB_P_HESS_REG, TSIDB_P_QUIRKS, TSIDB_P_NORMAL /*3*/,
  TSIDB_P_CPOINTS = TSIDB_P_NORMAL + 3 /*4x3*/, TSIDB_P_KP_POSTURE = TSIDB_P_CPOINTS + 12 /*20*/,
  TSIDB_P_KD_POSTURE = TSIDB_P_KP_POSTURE + 20, TSIDB_P_TAU_MAX = TSIDB_P_KD_POSTURE + 20,
  TSIDB_P_V_MAX = TSIDB_P_TAU_MAX + 20, TSIDB_P_MAX_ITER = TSIDB_P_V_MAX + 20, TSIDB_P_SIM_ENABLED, TSIDB_P_CLOSED_LOOP,
  TSIDB_P_W_AM /* angular-momentum task weight (legacy/biped.py:82-87), 0 = not in the stack */, TSIDB_P_KP_AM /*3*/,
  /* reward / done outputs (SURVEY.md 8d write list; no reference counterpart): reward = exp(-|com - com_ref|^2 / sigma^2)
   * - c_tau |tau|^2, done = failed QP, base height < DONE_HEIGHT or base z-axis . world z < DONE_TILT */
  TSIDB_P_REW_SIGMA = TSIDB_P_KP_AM + 3, TSIDB_P_REW_CTAU, TSIDB_P_DONE_HEIGHT, TSIDB_P_DONE_TILT,
  TSIDB_P_SELF_COLLISION /* sim: collide the robot<->robot hull pairs as mj_step does (main.py:195); 0 = floor only */,
  TSIDB_P_W_COP /* CoP force task weight (legacy/biped.py:79-80), 0 = not in the stack */,
  /* closed-loop knobs (all neutral by default = the reference's models): scale of the sim's joint
   * frictionloss (robot.xml:8), rotor inertia added to the diagonal of TSID's mass matrix on the actuated joints (the sim
   * has armature 0.005, the URDF none), Coulomb-friction feed-forward added to tau [N m] */
  TSIDB_P_SIM_FLOSS_SCALE, TSIDB_P_TSID_ARMATURE, TSIDB_P_FRICTION_COMP,
  /* sim: plane <-> mesh multi-contact rule (main.py:195, mj_step's plane-convex routine).  0: the support vertex plus EVERY
   * hull-graph neighbour of it within the margin; 1: upstream's rule as far as it is known here (mujoco is not available to
   * check): in graph order at most 3 more contacts, each at least 0.3 x the geom's bounding radius from the first */
  TSIDB_P_PLANE_MESH,
  TSIDB_P_COUNT = 128
};

/* WalkController.__init__ (ctrl/WalkController.py:12-187) + MjModel.from_xml_path (main.py:50-52):
 * parse the compiled model blob (include/tsidb_model.h), derive the constant QP blocks from
 * `params`, upload to `device`. */
int tsidb_create(const void *model_blob, size_t nbytes, const double *params, int n_params, int num_envs,
                 int device, int dtype, tsidb_handle *out);
int tsidb_destroy(tsidb_handle h);
const char *tsidb_last_error(tsidb_handle h);

/* RobotConfig edits after construction (the reference edits ctrl/conf.py and rebuilds).  First waits for the kernels in
 * flight on the streams this handle has launched on (on the whole device once there have been more than 32 of them), so
 * every stream a handle has launched on must outlive the handle or be released with tsidb_stream_destroy. */
int tsidb_set_params(tsidb_handle h, const double *params, int n_params);

/* task references: comTask.setReference (WalkController.py:152), postureTask.setReference (:165),
 * task_LF/RF.setReference (:195-196), contactLF/RF.setReference (:81,122,240,248), contact on/off
 * flags (:87,128,225,232,245,253), and the init-time frames get_cop reads (:77,281-282).
 * com_ref [N,9] pos vel acc; posture_ref [N,20]; foot_ref [N,2,24] = p(3) R col-major(9) v(6) a(6);
 * contact_ref [N,2,12] = p(3) R col-major(9); contact_active [N,2] u8; cop_frames [N,2,12] =
 * R row-major(9) p(3).  Pointers are remembered, not copied. */
int tsidb_set_refs(tsidb_handle h, const void *com_ref, const void *posture_ref, const void *foot_ref,
                   const void *contact_ref, const uint8_t *contact_active, const void *cop_frames);

/* execution options.  TSIDB_OPT_SIM_WAVES, TSIDB_OPT_LDS_PAD and TSIDB_OPT_CU_SPLIT leave every result bit-identical;
 * TSIDB_OPT_QP_FAST_EQ changes the tick's results within rounding.
 * TSIDB_OPT_SIM_WAVES: wavefronts per env in the sim kernel - 1 (one wavefront per env: the throughput-optimal shape once the
 * batch fills the GPU) or 2 (collision phase on a second wavefront beside the unconstrained dynamics: shorter step latency for
 * small batches).  Default: 2 for up to 512 envs, else 1.
 * TSIDB_OPT_LDS_PAD (diagnostic): bytes of unused dynamic LDS added to every k_tick / k_sim workgroup (0 .. 40960) - lowers the
 * number of resident workgroups per CU, for occupancy measurements; default 0.
 * TSIDB_OPT_CU_SPLIT: whether tsidb_stream_create hands out streams on disjoint halves of the CUs: 1 always, 0 never, -1 (default)
 * for up to 512 envs.
 * TSIDB_OPT_QP_FAST_EQ (default 1; float64, reference task stack): the tick first computes the equality-constrained optimum of
 * the QP by the range-space route (a Cholesky of the 6-18 x 6-18 matrix B^T B instead of the Householder QR applied to the
 * 26-50 x 26-50 factor) and runs the feasibility sweep there; an env with a violated inequality - or whose equality block is
 * ill conditioned (a pivot ratio below 1e-4) - continues with the QR and the dual active-set iterations exactly as with 0.  The
 * optimum is unique: results agree to rounding (1e-12 observed), status and iteration counts are the same. */
enum { TSIDB_OPT_SIM_WAVES = 1, TSIDB_OPT_LDS_PAD = 2, TSIDB_OPT_CU_SPLIT = 3, TSIDB_OPT_QP_FAST_EQ = 5 }; /* 4 is retired: never reuse it */
int tsidb_set_option(tsidb_handle h, int option, int value);
int tsidb_get_option(tsidb_handle h, int option, int *value); /* the EFFECTIVE setting (TSIDB_OPT_CU_SPLIT: 1 if tsidb_stream_create
                                                                * masks its streams for this handle's batch size) */

/* HIP streams for the pipelined step (tick of step t+1 on one stream beside the sim of step t on another; the reference couples
 * the two stages one way, main.py:119-129 vs :192-195).  While every wavefront of both kernels is resident at once (up to 512
 * envs: 2 x 512 wavefronts on 1024 SIMDs) the two kernels slow each other down when they share CU groups - k_tick 54 us alone,
 * 70 us beside a running k_sim - so the streams handed out here are restricted to disjoint halves of the device's CUs
 * (hipExtStreamCreateWithCUMask): + 11-14 % env-steps/s at 256 / 512 envs; above 512 envs (each kernel alone fills more than
 * half of the SIMDs) plain streams are returned.  role: TSIDB_STREAM_TICK / TSIDB_STREAM_SIM.  Results do not depend on it. */
enum { TSIDB_STREAM_TICK = 0, TSIDB_STREAM_SIM = 1 };
int tsidb_stream_create(tsidb_handle h, int role, void **stream);
int tsidb_stream_destroy(tsidb_handle h, void *stream);

/* reference point of the CoP force task (legacy/biped.py:79-80 copTask; params[W_COP] != 0): cop_ref [N,3], world
 * frame; written by tsidb_reset (midpoint of the soles on the floor).  The pointer is remembered, not copied. */
int tsidb_set_cop_ref(tsidb_handle h, const void *cop_ref);

/* per-env randomisation of the sim stage (BASELINE.json configs[4]; no reference counterpart):
 * env_params [N,8] in the path's arithmetic type = mass scale applied to every sim body's mass and inertia,
 * contact friction, unit floor normal (3), floor offset d (plane n.x = d), 2 spare.  NULL = nominal
 * model (floor z = 0, friction 1).  terrain [N,20] (may be NULL = flat) = stepped floor: direction (2, unit, world xy),
 * phase, 1 / step length, heights[16] - the floor surface is raised along its normal by heights[cell & 15] with
 * cell = floor((direction . x_world_xy - phase) / step length) ("rough-terrain contacts", 1 cm steps).  The pointers
 * are remembered, not copied. */
int tsidb_set_env_params(tsidb_handle h, const void *env_params, const void *terrain);

/* external body wrenches of the sim stage: mj_data.xfrc_applied, the field a caller of mj_step (main.py:195) writes to push
 * the robot.  xfrc [N, NB, 6] (device, the path's arithmetic type; NB = sim bodies, tsidb_dims out9[4]) in the blob's sim body
 * order - mj_parent order, MJCF document order without the world body, body 0 = the torso with the free joint - so
 * xfrc[e, b] is xfrc_applied[b + 1] of env e.  Each row is force (3) then torque (3), both in the world frame, applied at the
 * body's centre of mass.  As in MuJoCo the values persist until the caller changes them: every sim step reads them (every
 * step of a tsidb_sim_batch launch, every substep of tsidb_step).  They enter the smooth force (qfrc_smooth += sum_b J_b^T
 * w_b): the unconstrained acceleration, the contact solve and the damped-Euler integration all see them.  In the open-loop
 * teleport mode (main.py:192 overwrites the base pose every step) a wrench on the torso moves it for that one step only;
 * pushes on limbs do act.  A non-finite value skips the env's step like a non-finite joint target (info flag bit 4).
 * tsidb_reset / tsidb_reset_done zero the rows of the envs they reset (mj_resetData).  NULL (the default) = no external
 * wrenches.  Rejected by a library built without the sim stage.  The pointer is remembered, not copied. */
int tsidb_set_xfrc(tsidb_handle h, void *xfrc);

/* direct actuator control of the sim stage: mj_data.ctrl, the field a caller of mj_step (main.py:195) writes to drive the
 * actuators - a policy's joint targets or torques, a residual on top of TSID, replayed commands.  ctrl [N, NA] (device, the
 * path's arithmetic type) in the MJCF actuator order, the order of act_force (tsidb_set_sim_readouts): actuator a drives the
 * joint whose TSID position is q[mj_ctrl_qidx[a]] (the blob's section).  As in MuJoCo the values persist until the caller
 * changes them: every sim step reads them anew (tsidb_sim, every step of a tsidb_sim_batch launch, every substep of
 * tsidb_step, every step of tsidb_sim_ctrl).  mode says what a value is; with d the actuator's dof:
 *   TSIDB_CTRL_POSITION  a joint target [rad] for the model's <position> servo, force = clampF(kp (clampC(ctrl) - q_d) - kv qdot_d)
 *                        with its ctrlrange / forcerange clamps - what mj_step does with mj_data.ctrl.  Replaces the target
 *                        taken from q_tsid, and replaces tau in the closed loop.
 *   TSIDB_CTRL_MOTOR     a motor torque [N m], applied unclamped exactly as the closed loop applies tau.  Replaces the servo in
 *                        the open loop and tau in the closed loop.
 *   TSIDB_CTRL_RESIDUAL  an offset to the control signal the TSID stage supplies.  In a step driven by position targets a
 *                        target offset [rad]: clampC(target + ctrl), target = 0 when q_tsid is NULL; in a step driven by tau
 *                        (closed loop) a torque offset [N m]: tau + ctrl.  An all-zero buffer leaves every result bit-identical.
 * The base teleport stays what q_tsid decides: ctrl only decides the joints.  In POSITION / MOTOR mode the closed-loop
 * tsidb_step still runs the tick and writes tau, but the sim is driven by ctrl.  The act_force readout reports the force
 * applied, in every mode.  A non-finite value skips the env's step like a non-finite joint target (info flag bit 4).
 * tsidb_reset / tsidb_reset_done zero the rows of the envs they reset (mj_resetData).  NULL with TSIDB_CTRL_OFF (the default)
 * unregisters: the sim is driven by q_tsid / tau alone, by the kernels that do not read ctrl.  Fails (message via
 * tsidb_last_error) for an unknown mode, for NULL with another mode than TSIDB_CTRL_OFF or a buffer with TSIDB_CTRL_OFF, and in a
 * library built without the sim stage.  Changing the registration first waits for the handle's kernels in flight, as
 * tsidb_set_sensors does.  The pointer is remembered, not copied. */
enum { TSIDB_CTRL_OFF = 0, TSIDB_CTRL_POSITION = 1, TSIDB_CTRL_MOTOR = 2, TSIDB_CTRL_RESIDUAL = 3 };
int tsidb_set_ctrl(tsidb_handle h, void *ctrl, int mode);

/* sim-stage readouts of the last sim step (mj_data.contact, mj_contactForce, mj_data.actuator_force); each may be NULL.
 * con_force [N,32,6], con_frame [N,32,9], con_pos [N,32,4] = world position (3) + dist,
 * act_force [N,NA], foot_grf [N,2,6] = world force (3) + CoP (3).  Rows >= ncon are zero.
 * Device buffers in the path's arithmetic type.  Contact c is row c of con_pairs, in the same order.  con_force is
 * mj_contactForce: normal, tangent 1, tangent 2, torsional (contact dimension 4 only, else 0), 0, 0 in the contact frame, the
 * force geom1 exerts on geom2, decoded from the pyramid rows at the solver's final acceleration.  The frame's rows are the
 * normal, pointing from geom1 to geom2, and the two tangents (contact.frame; mju_makeFrame).  The floor is geom1 of every
 * floor contact, so the normal points up out of the floor and the force is the floor's push on the robot.  con_pos is
 * contact.pos and contact.dist, taken where the step's collision ran (its start).  act_force is actuator_force in the MJCF
 * actuator order (the ctrl order): the clamped position-servo force, or the motor torque in the closed loop (with
 * tsidb_set_ctrl: the force that mode applied).  foot_grf holds
 * per sole (LF, RF, TSID's contact order) the floor contacts on that sole's sim body summed in the world frame, then their
 * centre of pressure (normal-force-weighted mean of the contact positions; all zero while the sole carries no normal force).
 * Every sim step writes them (a tsidb_sim_batch launch or a tsidb_step with substeps leaves the last step's values); a
 * skipped step (info flag bit 4) zeroes the env's rows.  tsidb_reset / tsidb_reset_done do not touch them, as they leave
 * ncon and con_pairs alone.  The pointers are remembered, not copied; all NULL (the default) unregisters.  Rejected by a
 * library built without the sim stage. */
int tsidb_set_sim_readouts(tsidb_handle h, void *con_force, void *con_frame, void *con_pos, void *act_force, void *foot_grf);

/* site sensors of the sim stage: mj_data.sensordata, which mj_step fills through mj_sensorPos / mj_sensorVel / mj_sensorAcc
 * (robot/v0/robot.xml:214-219 declares framepos, framequat, framelinvel and frameangvel on root_site).  n_sites sites
 * (1 .. TSIDB_MAXSITE): site_body [S] (the blob's sim body order, as for tsidb_set_xfrc), site_pos [S,3] and site_quat [S,4]
 * (wxyz, normalised on the way in) in the body's own frame - host arrays, copied into the model constants.  sensordata
 * [N,S,TSIDB_NSENS] is a device buffer in the path's arithmetic type; the pointer is remembered, not copied.  Row per site:
 *   0-2   framepos      world position of the site (mj_sensorPos: site_xpos)
 *   3-6   framequat     world orientation, wxyz, unit; w >= 0 is not enforced, as in MuJoCo (mj_sensorPos)
 *   7-9   framelinvel   world-frame linear velocity of the site point (mj_sensorVel: mj_objectVelocity, flg_local = 0)
 *   10-12 frameangvel   world-frame angular velocity (the same call)
 *   13-15 velocimeter   linear velocity in the site frame (mj_sensorVel: mj_objectVelocity, flg_local = 1)
 *   16-18 gyro          angular velocity in the site frame (the same call)
 *   19-21 accelerometer site-frame linear acceleration of the site point minus gravity (mj_sensorAcc: mj_objectAcceleration on
 *                       the cacc of mj_rnePostConstraint, whose world body accelerates at -gravity; it includes the omega x v
 *                       term that turns the spatial into the classical acceleration): R_site^T (0,0,+g) at rest on the floor,
 *                       0 in free fall.  The acceleration is the constraint solver's qacc (mj_data.qacc, what the step leaves
 *                       in qacc_ws) - with joint damping (the v0 robot) not the damped-Euler effective one.
 *   22-23 spare         zero
 * Timing is mj_step's: sensors are evaluated inside mj_forward, before the integrator, so after a step the rows describe the
 * positions and velocities the step STARTED from (in the teleport mode: after the teleport) and the acceleration it solved for.
 * Every sim step writes the rows (a tsidb_sim_batch launch or a tsidb_step with substeps leaves the last step's values); a
 * skipped step (info flag bit 4) zeroes the env's rows; tsidb_reset / tsidb_reset_done do not touch them.  n_sites = 0 with
 * sensordata = NULL (the default) unregisters.  Changing the site table first waits for the handle's kernels in flight, as
 * tsidb_set_params does.  Fails (message via tsidb_last_error) in a library built without the sim stage, for a body index out
 * of range, a non-finite value, a zero quaternion, more than TSIDB_MAXSITE sites, and when exactly one of n_sites and
 * sensordata is empty. */
enum { TSIDB_MAXSITE = 16, TSIDB_NSENS = 24 };
int tsidb_set_sensors(tsidb_handle h, int n_sites, const int32_t *site_body, const double *site_pos, const double *site_quat,
                      void *sensordata);

/* reset: WalkController.py:22-26,72-79 (standing state, soles onto z = 0), the references of
 * :81,122,151-152,164-165, and main.py:57-64 (mj_data.qpos = q).  env_ids (device, int32) selects
 * envs; NULL = all (a non-NULL list with n_ids = 0 resets nothing).  Writes state AND the reference buffers
 * registered with tsidb_set_refs. */
int tsidb_reset(tsidb_handle h, const int32_t *env_ids, int n_ids, void *q, void *v, void *qpos, void *qvel,
                void *qacc_ws, void *stream);

/* one TSID tick for every env: main.py:119-129 (+ readouts :132-142).
 * q [N,27], v [N,26] updated in place; tau [N,20], dv [N,26], f [N,24] (LF 12, RF 12), status [N],
 * obs [N,obs_ld] = q v com cop LF RF (65 values; may be NULL; obs_ld >= 65 is the row stride in elements -
 * with obs_ld >= TSIDB_NROW columns 65, 66 receive reward and done, so that one contiguous [N,67] buffer is
 * what the all-gather sends), frames [N,2,12] sole placements R row-major + p (may be NULL), info [N,4]
 * int32 = qp iterations, active-set size, -, - (may be NULL). */
int tsidb_tick(tsidb_handle h, void *q, void *v, void *tau, void *dv, void *f, int32_t *status, void *obs,
               int obs_ld, void *frames, int32_t *info, void *stream);

/* one sim step for every env: main.py:192-195.  q_tsid [N,27] (NULL = no teleport, ctrl = 0); v_tsid
 * [N,26] (may be NULL) is used only with params[QUIRKS] = 0: the base velocity is then set together with
 * the base pose (the reference writes qpos[:7] only, which leaves the sim's base velocity to drift once
 * the TSID state moves).  qpos [N,27], qvel [N,26], qacc_ws [N,26] updated in place; qacc [N,26], ncon [N],
 * con_pairs [N,32] = (geom << 16 | hull vertex) for floor contacts, (geom2 << 16 | 0x8000 | geom1) for robot<->robot
 * ones, -1 padded (geom = collision geom in the blob's order; the v1 robot has one per body, in body order);
 * info [N,4] slots 2,3 = solver iterations, flag bits (all may be NULL).  Flag bits: 1 the damped-Euler matrix, 2 the Newton
 * Hessian was not positive definite (the step ends with what it has); 4 the step was skipped (non-finite or diverged state /
 * targets); 8 a penetrating contact was dropped at a cap (TSIDB_MAXCON contacts per env, 12 of them robot<->robot);
 * 16 a support vertex has more than 63 hull-graph neighbours (the rest is not looked at); 32 more than 64 candidate pairs
 * survived the mid phase (the rest is not collided). */
int tsidb_sim(tsidb_handle h, const void *q_tsid, const void *v_tsid, void *qpos, void *qvel, void *qacc_ws,
              void *qacc, int32_t *ncon, int32_t *con_pairs, int32_t *info, void *stream);

/* n_steps (1 .. TSIDB_MAX_SIM_BATCH) consecutive sim steps in ONE launch: step b teleports to / takes its joint targets from
 * slot slots[b] (host array, 0 .. 15) of the snapshot rings q_ring [K,N,27], v_ring [K,N,26] (v_ring may be NULL) - what n_steps
 * calls of tsidb_sim with q_tsid = q_ring[slots[b]] do, without the launch gaps between them (the pipelined open-loop step
 * hands over the TSID states of several ticks at once; envs do not interact, so each steps on its own).  Bit for bit, in
 * float64 and float32: the library is built with -ffp-contract=on, so the separately compiled instantiations of the sim kernel
 * (single- / multi-step, one / two wavefronts per env, two envs per wavefront) fuse exactly the multiply-adds the source writes
 * as one expression (with hipcc's default, fast, the multi-step kernel differed from the single-step one by 1 ulp in float32
 * after 231 walking steps; tests: test_shard_invariance_across_kernel_shapes).
 * ncon / con_pairs / info are the last step's. */
enum { TSIDB_MAX_SIM_BATCH = 8 };
int tsidb_sim_batch(tsidb_handle h, int n_steps, const void *q_ring, const void *v_ring, const int32_t *slots, void *qpos, void *qvel,
                    void *qacc_ws, void *qacc, int32_t *ncon, int32_t *con_pairs, int32_t *info, void *stream);

/* n_steps (1 .. TSIDB_MAX_SIM_BATCH) consecutive sim steps in ONE launch, driven by the registered ctrl buffer (tsidb_set_ctrl)
 * alone: no teleport, no TSID state - what n_steps calls of tsidb_sim with q_tsid = NULL do, bit for bit (see tsidb_sim_batch),
 * without the launch gaps between them.  ctrl is held over the steps (zero-order hold), so a policy can run at a fraction of the
 * sim's rate.  ncon / con_pairs / info, the readouts and the sensors are the last step's.  Fails while no buffer is registered. */
int tsidb_sim_ctrl(tsidb_handle h, int n_steps, void *qpos, void *qvel, void *qacc_ws, void *qacc, int32_t *ncon, int32_t *con_pairs,
                   int32_t *info, void *stream);

/* whole env step, n_substeps times: tsidb_tick then (if params[SIM_ENABLED]) tsidb_sim.
 * With params[CLOSED_LOOP] (not in the reference, whose coupling is one-way, main.py:126-129,
 * 192-195): each tick first reads the TSID state from the sim state (quat wxyz -> xyzw, world-frame base
 * linear velocity -> body frame, sim joint order -> TSID order), and the sim stage applies tau as motor
 * torques and keeps its own base pose instead of the teleport + position servos. */
int tsidb_step(tsidb_handle h, void *q, void *v, void *qpos, void *qvel, void *qacc_ws, void *tau, void *dv,
               void *f, int32_t *status, void *obs, int obs_ld, void *frames, int32_t *ncon, int32_t *con_pairs,
               int32_t *info, int n_substeps, void *stream);

/* walking reference update for every env, on the device (config 3): what the reference's main.py:117
 * intends with controller.update_tasks(sampleLF, sampleRF, contact_LF, contact_RF) when the samples
 * come from ctrl/Walk_Planner.py:23-31 swing trajectories (ctrl/Foot_Trajectory.py polynomials) over
 * a ctrl/Footstep_Planner.py plan.  coef [N,K,4,4] = x, y, z, yaw cubic coefficients (ascending, in
 * time since the step started); side [N,K] int32 = swinging foot of step k (0 left); nsteps [N] int32;
 * rest [N,K+1,2,4] = (x, y, yaw, z) of [left, right] foot before step k; com [N,K+2,2,3] = linear-inverted-
 * pendulum segment (zmp, d, c) per planar axis for the start phase, each step and the final stand
 * (ctrl/LIPM.py:34-49 about a fixed ZMP, in closed form x(s) = zmp + d/2 e^{omega s} + c e^{-omega s}).
 * Timeline: [0, t_start) both feet down while the CoM height goes from com_z0 to com_z0 - com_drop; step
 * k occupies [t_start + k T, t_start + (k+1) T); afterwards both feet are down.  Writes the registered
 * foot_ref / contact_ref / contact_active / com_ref (position, velocity, acceleration) buffers; contact
 * on/off edges re-reference at `frames` [N,2,12] (current sole placements from the last tsidb_tick), as
 * ctrl/WalkController.py:215-253 intends.  t_offset [N] (may be NULL) delays each env's timeline: env e runs
 * on the clock max(t - t_offset[e], 0), so that the envs of one batch need not step in phase.  Contact-timing
 * feedback (closed loop; td_latch [N] int32, initialised to -1, may be NULL = off): when the last sim step's contact
 * list (ncon, con_pairs of tsidb_sim / tsidb_step) shows the swing foot on the floor after td_fraction of its
 * swing, the touch-down is taken at once - the foot is a stance foot for the rest of that step.  t_device (may be
 * NULL): one float64 value (whatever the path's arithmetic type) in device memory that replaces `t` - the launch can
 * then be captured in a HIP graph and replayed while the caller advances the clock on the device. */
int tsidb_walk_update(tsidb_handle h, const void *coef, const int32_t *side, const int32_t *nsteps,
                      const void *rest, const void *com, int K, double t, double step_duration, double t_start,
                      double omega, double com_z0, double com_drop, const void *frames, const void *t_offset,
                      const int32_t *ncon, const int32_t *con_pairs, int32_t *td_latch, double td_fraction,
                      const void *t_device, void *stream);

/* ---- episode lifecycle on the device (SURVEY.md 8f-2, section 5 "auto-reset mask"; no reference counterpart: the reference
 * runs one episode and exits, main.py:113-124) */

/* tsidb_reset for exactly the envs whose done flag is set: rows [N, rows_ld >= TSIDB_NROW] as tsidb_tick wrote them
 * (done in column TSIDB_NOBS + 1) - no host round trip between `done` and the restart.  frames (may be NULL) [N,2,12]
 * receives the reset envs' sole placements (what the next tsidb_walk_update re-references contacts at). */
int tsidb_reset_done(tsidb_handle h, const void *rows, int rows_ld, void *q, void *v, void *qpos, void *qvel, void *qacc_ws,
                     void *frames, void *stream);

/* [NA] values (the path's arithmetic type, device) added to the posture reference every reset captures
 * (ctrl/WalkController.py:164-165 takes q0's joints; a walking workload keeps its knees bent).  NULL = none.  The pointer
 * is remembered, not copied. */
int tsidb_set_posture_bias(tsidb_handle h, const void *posture_bias);

/* Episode plan for the selected envs, built on the device: env_ids (device int32, NULL = all) and / or done_rows (as for
 * tsidb_reset_done: only envs whose done flag is set).  For each: footsteps along its path (ctrl/Footstep_Planner.py:92-125),
 * swing polynomials from footstep k to k + 2 (ctrl/Walk_Planner.py:23-31, ctrl/Foot_Trajectory.py:5-27), rest placements and
 * the LIPM / DCM CoM plan (ctrl/LIPM.py:34-49 in closed form) - the tables tsidb_walk_update reads (layouts there), starting
 * from the sole placements and the CoM that tsidb_reset left in the registered cop_frames / com_ref buffers.
 * plan_params [TSIDB_PLAN_NPARAMS] (host): step_length, step_width, step_height, step_duration, rise_ratio
 * (ctrl/conf.py:24-28), t_start, com_drop, foot_press (every swing is aimed this far below the floor), resample_ds (path
 * vertices at most this far apart before planning; 0 = as given), unicycle path v, w, dt, n (Footstep_Planner.py:131-141),
 * scale_lo, scale_hi, seed.  Path per env: `path` [N,P,2] float64 + npts [N] = an explicit polyline in world coordinates,
 * used as given; NULL = the unicycle path scaled by scale[e] ([N] float64) or, with scale NULL and episode [N] int32 given,
 * by U(scale_lo, scale_hi) drawn from hash(seed, env, episode[e]) (bump_episode != 0 increments episode[e] first), rotated
 * into the robot's heading and started between its feet.  Outputs: steps [N,K+2,4] float64 = x, y, yaw, side of every
 * footstep (the two initial ones first); nsteps [N]; coef, side, rest, com as tsidb_walk_update reads them; flags [N] (may
 * be NULL) bit 0 = the plan needed more than K steps and was cut, bit 1 = the path had no direction (fewer than two distinct
 * vertices; npts[e] is clamped to P): no step planned, the env stands; bit 2 = a path piece longer than 4096 resample intervals
 * (or with a non-finite vertex) was resampled coarser; bit 3 (with bit 1) = the CoM is not above the feet after the descent
 * (com_ref[2] - com_drop <= 1 mm: plan before a reset, or com_drop >= the standing height): no step planned, finite tables.
 * Rejected by the call (error): non-finite parameters, step_width <= 0, resample_ds in (0, step_length / 1000), a unicycle
 * path of more than 65536 vertices or with dt <= 0, a scale range that is not 0 < lo <= hi.  The env's clock restarts: t_offset [N] (may be NULL)
 * receives `t` (or *t_device, float64 device), td_latch [N] (may be NULL) -1. */
enum { TSIDB_PLAN_NPARAMS = 16 };
int tsidb_walk_plan(tsidb_handle h, const int32_t *env_ids, int n_ids, const void *done_rows, int rows_ld,
                    const double *plan_params, int n_plan_params, const double *path, const int32_t *npts, int P,
                    const double *scale, int32_t *episode, int bump_episode, int K, double *steps, void *coef, int32_t *side,
                    int32_t *nsteps, void *rest, void *com, int32_t *flags, void *t_offset, int32_t *td_latch, double t,
                    const double *t_device, void *stream);

/* tsidb_walk_update's arguments as one block (same meaning, same order) */
typedef struct tsidb_walk_args {
  const void *coef; const int32_t *side; const int32_t *nsteps; const void *rest; const void *com; int K;
  double t, step_duration, t_start, omega, com_z0, com_drop;
  const void *frames; const void *t_offset; const int32_t *ncon; const int32_t *con_pairs; int32_t *td_latch; double td_fraction;
  const double *t_device;
} tsidb_walk_args;

/* tsidb_tick with two fusions for the tick stream of a pipelined step (what bounds small batches: three launches less):
 * walk (may be NULL): this tick's walking reference update (exactly tsidb_walk_update(walk...), run per env in the tick kernel's
 * prologue: controller.update_tasks(...) of main.py:117 and formulation.computeProblemData of main.py:119 in one launch);
 * q_snapshot / v_snapshot (may be NULL) [N,27] / [N,26]: a second copy of the TSID state the tick ends on, for a sim stage that
 * runs on another stream while the next tick already overwrites q / v.  Results are those of the separate calls, bit for bit. */
int tsidb_tick_walk(tsidb_handle h, const tsidb_walk_args *walk, void *q, void *v, void *tau, void *dv, void *f, int32_t *status,
                    void *obs, int obs_ld, void *frames, int32_t *info, void *q_snapshot, void *v_snapshot, void *stream);

/* ---- the environment around a policy-driven sim loop (no reference counterpart: the reference's only controller is TSID).
 * One policy step is tsidb_policy_act, tsidb_sim_ctrl (decimation sim steps), tsidb_policy_reward, tsidb_reset_done,
 * tsidb_policy_obs on one stream: plain asynchronous launches, no host synchronisation, no allocation, so the step can be
 * captured in a HIP graph.  All three fail (message via tsidb_last_error) in a library built without the sim stage, while no
 * ctrl buffer is registered (tsidb_set_ctrl) and before tsidb_policy_config.  The TSIDB_POL_NOBS constant is the v1 robot's:
 * 11 + 3 NA in general (65 for robot/v0).
 *
 * Reward terms, unweighted, in the order of terms [N, TSIDB_POL_NT] and of the weights; v = R^T qvel[0:3] and w = qvel[3:6] are
 * the base velocities in the body frame (quaternion stored wxyz, normalised on the way in), g = R^T (0, 0, -1) the projected
 * gravity, cmd = command[e] = (vx, vy, yaw rate):
 *   0 track_lin_vel  exp(-|cmd_xy - v_xy|^2 / sigma^2)        6 torques        sum_a act_force_a^2 (0 while no act_force readout
 *   1 track_ang_vel  exp(-(cmd_yaw - w_z)^2 / sigma^2)                         is registered, tsidb_set_sim_readouts)
 *   2 lin_vel_z      v_z^2                                    7 action_rate    sum_a (last_action_a - prev_action_a)^2
 *   3 ang_vel_xy     w_x^2 + w_y^2                            8 joint_vel      sum_a qvel[mj_act_dof[a]]^2
 *   4 orientation    g_x^2 + g_y^2                            9 feet_air_time  sum_f (air_f - t_air) first_contact_f [|cmd_xy| > deadband]
 *   5 base_height    (z - h_target)^2                         10 alive 1       11 termination  1 if terminated else 0 */
enum { TSIDB_POL_NT = 12, TSIDB_POL_HIST = 8, TSIDB_POL_NOBS = 71, TSIDB_POL_NPRIV = 4 };

/* tsidb_policy_config's parameter vector (float64, host) */
enum {
  TSIDB_POL_P_CLIP = 0 /* actions are clipped to +-clip (>= 0) */, TSIDB_POL_P_ALPHA /* ctrl filter, in (0, 1]; 1 = none */,
  TSIDB_POL_P_SIGMA /* of both tracking terms, > 0 */, TSIDB_POL_P_H_TARGET, TSIDB_POL_P_T_AIR, TSIDB_POL_P_DEADBAND,
  TSIDB_POL_P_MAX_EPISODE_STEPS /* policy steps until the timeout; 0 = none */, TSIDB_POL_P_DECIMATION /* sim steps per policy step, >= 1 */,
  TSIDB_POL_P_SEED /* of the command draws */, TSIDB_POL_P_CMD_LO /*3*/, TSIDB_POL_P_CMD_HI = TSIDB_POL_P_CMD_LO + 3 /*3*/,
  TSIDB_POL_P_WEIGHTS = TSIDB_POL_P_CMD_HI + 3 /*TSIDB_POL_NT*/, TSIDB_POL_NPARAMS = TSIDB_POL_P_WEIGHTS + TSIDB_POL_NT
};

/* Copies pol_params [TSIDB_POL_NPARAMS], scale [NA] and default_pos [NA] (host, float64, MJCF actuator order) and
 * term_body_mask (bit b: a floor contact on sim body b ends the episode; the blob's sim body order, 0 = the torso) into the
 * handle.  First waits for the kernels in flight, as tsidb_set_params does.  Rejects a wrong n_params, non-finite values, clip < 0,
 * alpha outside (0, 1], sigma <= 0, decimation < 1, max_episode_steps < 0, cmd_lo > cmd_hi and a mask bit >= the number of sim
 * bodies. */
int tsidb_policy_config(tsidb_handle h, const double *pol_params, int n_params, const double *scale, const double *default_pos,
                        uint32_t term_body_mask);

/* the per-env state of the policy environment: device buffers owned by the caller, in the path's arithmetic type unless an
 * integer type is named; all but delay and obs are required */
typedef struct tsidb_policy_bufs {
  void *act_hist;     /* [TSIDB_POL_HIST, N, NA] ring of clipped actions, slot = episode step & 7 */
  void *last_action;  /* [N, NA] */
  void *prev_action;  /* [N, NA] */
  void *command;      /* [N, 3] vx, vy, yaw rate; redrawn at a restart where cmd_lo != cmd_hi, else the caller's */
  void *air_time;     /* [N, 2] seconds since the left / right sole last touched the floor */
  int32_t *ep_len;    /* [N] policy steps taken in the running episode */
  int32_t *episode;   /* [N] episodes started */
  const int32_t *delay; /* [N] actuation delay in policy steps, clamped to 0 .. 7; NULL = none */
  void *terms;        /* [N, TSIDB_POL_NT] the unweighted reward terms of the last tsidb_policy_reward */
  int32_t *timeout;   /* [N] 1 where the last step ended the episode by its length alone */
  void *obs;          /* [N, obs_ld]; NULL = tsidb_policy_obs writes no rows */
  int obs_ld;         /* row stride in elements, >= TSIDB_POL_NOBS + TSIDB_POL_NPRIV */
} tsidb_policy_bufs;

/* before the sim steps.  Per env e and actuator a (the order of ctrl): act = clip(action, +-clip), a NaN passing through (the sim
 * step then skips the env, info flag bit 4, which tsidb_policy_reward counts as a termination); act_hist[ep_len & 7] = act;
 * delayed = the ring entry from delay[e] steps ago, 0 where delay[e] > ep_len[e]; target = default[a] + scale[a] delayed;
 * ctrl += alpha (target - ctrl), exactly target when alpha = 1; prev_action = last_action, last_action = act.  ctrl is the
 * registered buffer; whether its values are joint targets or torques is tsidb_set_ctrl's mode.  action [N, NA] (device). */
int tsidb_policy_act(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *action, void *stream);

/* after the sim steps, before the reset: qpos, qvel, ncon, con_pairs, info as tsidb_sim_ctrl left them.  Writes terms, reward =
 * sum_k weights[k] terms[k], done and timeout, then the air times and ep_len += 1.  reward and done point at the first env's
 * values, row_ld elements apart (columns TSIDB_NOBS and TSIDB_NOBS + 1 of the rows tsidb_reset_done reads).  The foot contact
 * flag c_f is 1 when a live floor row of con_pairs (bit 0x8000 clear) is on a geom of sole f's body; first_contact_f = c_f and
 * air_f > 0; afterwards air_f = c_f ? 0 : air_f + decimation dt.  terminated: info flag bit 4, a non-finite state,
 * z < params[DONE_HEIGHT], 1 - 2 (qx^2 + qy^2) < params[DONE_TILT] (tsidb_tick's fall test on the sim quaternion) or a floor
 * contact on a body of term_body_mask; timeout = not terminated and max_episode_steps > 0 and ep_len + 1 >= max_episode_steps;
 * done = terminated or timeout. */
int tsidb_policy_reward(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *qpos, const void *qvel, const int32_t *ncon,
                        const int32_t *con_pairs, const int32_t *info, void *reward, void *done, int row_ld, void *stream);

/* after tsidb_reset_done(done_rows, ...).  Envs whose done flag is set (column TSIDB_NOBS + 1 of done_rows [N, rows_ld]): ring
 * rows, last_action, prev_action, air_time and ep_len zeroed, episode + 1, the ctrl row set to default in TSIDB_CTRL_POSITION
 * mode (the filter starts at the default pose; the reset left 0, which stays in the other modes), and command[i] = lo_i +
 * (hi_i - lo_i) U_i where cmd_lo[i] != cmd_hi[i], U_i = the top 53 bits of hash(seed + i, env, episode) - the hash of
 * tsidb_walk_plan - over 2^53.  Then for every env the observation row from the current state, physical units, unscaled:
 *   0-2 base angular velocity (body frame)   3-5 projected gravity   6-8 command   9.. joint position - default (NA, actuator
 *   order: qpos[mj_act_dof[a] + 1])   then joint velocity (NA: qvel[mj_act_dof[a]])   then last_action (NA)   then the foot
 *   contact flags LF, RF ((1, 1) for an env just reset: the reset leaves the contact list of the fallen robot)   then the
 *   privileged tail from column TSIDB_POL_NOBS: base linear velocity (body frame, 3), base height. */
int tsidb_policy_obs(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld, const void *qpos,
                     const void *qvel, const int32_t *ncon, const int32_t *con_pairs, void *stream);

/* ---- randomisation of the policy environment: per-episode reset noise, per-step observation noise, pushes and command
 * resampling, all on the device and all off by default.  No random state is stored anywhere: every draw is
 *   U = (hash(key, env_offset + env, counter) >> 11) / 2^53   in float64 whatever the path's type,
 * hash = the one of tsidb_walk_plan and of the restart command draw above, so a draw is a pure function of (seed, stream, column,
 * env, episode, ep_len): a captured graph replays it, and a batch split over ranks (env_offset = the rank's first env) draws
 * what the unsplit batch draws.  Symmetric noise is amp (2 U - 1), formed in float64, cast to the path's type, then added.
 *
 * Key layout: key = seed + ((stream * 256 + column) * 2^32), seed = TSIDB_POL_DR_SEED below 2^32, stream >= 1, column < 256.  No
 * two (stream, column) pairs share a key, and none equals the restart command draw's keys TSIDB_POL_P_SEED + (0, 1, 2) while that
 * seed is below 2^32 as well.  Streams, their column and their counter (episode and ep_len are the env's entries of
 * tsidb_policy_bufs):
 *   stream  draw                     column              counter
 *   1       reset joint position     actuator            the episode about to start (episode + 1 when the kernel runs)
 *   2       reset joint velocity     actuator            same
 *   3       reset base lin velocity  component x, y, z   same
 *   4       reset base ang velocity  component x, y, z   same
 *   5       reset yaw                -                   same
 *   6       reset x, y               component x, y      same
 *   7       observation noise        observation column  episode * 2^32 + ep_len, both as tsidb_policy_obs leaves them
 *   8       push phase               -                   episode
 *   9       push magnitude           -                   episode * 2^32 + k, k = the number of the push in the episode
 *   10      push azimuth             -                   same
 *   11      command zeroing          -                   episode + k * 2^32, k = the number of the resample (0 = the restart)
 * The command components themselves keep their keys TSIDB_POL_P_SEED + i and use the counter episode + k * 2^32: resample 0 is
 * the restart draw described at tsidb_policy_obs.  env_offset enters every draw, that one included. */
enum {
  TSIDB_POL_DR_SEED = 0 /* integer in [0, 2^32) */, TSIDB_POL_DR_ENV_OFFSET /* integer in [0, 2^31) */,
  TSIDB_POL_DR_RESET_JOINT_POS /* rad */, TSIDB_POL_DR_RESET_JOINT_VEL /* rad/s */, TSIDB_POL_DR_RESET_BASE_LIN_VEL /*3, m/s, world*/,
  TSIDB_POL_DR_RESET_BASE_ANG_VEL = TSIDB_POL_DR_RESET_BASE_LIN_VEL + 3 /*3, rad/s, as qvel stores it*/,
  TSIDB_POL_DR_RESET_YAW = TSIDB_POL_DR_RESET_BASE_ANG_VEL + 3 /* rad */, TSIDB_POL_DR_RESET_XY /* m */,
  TSIDB_POL_DR_RESET_LIFT /* m, added to base z, not random */,
  TSIDB_POL_DR_NOISE_ANG_VEL, TSIDB_POL_DR_NOISE_GRAVITY, TSIDB_POL_DR_NOISE_JOINT_POS, TSIDB_POL_DR_NOISE_JOINT_VEL,
  TSIDB_POL_DR_PUSH_INTERVAL /* policy steps; 0 = no pushes */, TSIDB_POL_DR_PUSH_DURATION /* policy steps */,
  TSIDB_POL_DR_PUSH_FORCE_LO /* N */, TSIDB_POL_DR_PUSH_FORCE_HI,
  TSIDB_POL_DR_COMMAND_INTERVAL /* policy steps; 0 = commands change at restarts only */, TSIDB_POL_DR_COMMAND_ZERO_PROB,
  TSIDB_POL_DR_NPARAMS
};

/* Copies dr_params [TSIDB_POL_DR_NPARAMS] (host, float64) into the handle; NULL with n_params 0 switches every group off again
 * (all values 0, the state of a new handle).  First waits for the kernels in flight, as tsidb_policy_config does.  Rejects a
 * wrong n_params, non-finite values, a negative amplitude, force, interval, seed or offset, a seed >= 2^32, an offset or interval
 * >= 2^31, push_duration > push_interval, push_force_lo > push_force_hi and a command_zero_prob outside [0, 1]; nothing of a
 * rejected vector is taken. */
int tsidb_policy_randomize(tsidb_handle h, const double *dr_params, int n_params);

/* before the sim steps (after or before tsidb_policy_act): the push of this policy step into the torso force xfrc[e, 0, 0:3] of
 * the buffer registered with tsidb_set_xfrc; every other element of xfrc is the caller's.  Per env, with len = ep_len[e] (the
 * policy steps completed in the episode: the value before tsidb_policy_reward increments it) and P = push_interval:
 * phase = floor(U_phase P); for len >= phase, k = (len - phase) / P and r = (len - phase) % P, and the push is active iff
 * r < push_duration.  An active push is F = m (cos a, sin a, 0) with m = lo + (hi - lo) U_mag(k), a = 2 pi U_azimuth(k), formed
 * in float64 and cast; an inactive one writes 0.  Written every step.  Fails while no xfrc buffer is registered; launches nothing
 * and succeeds while push_interval or push_duration is 0. */
int tsidb_policy_perturb(tsidb_handle h, const tsidb_policy_bufs *bufs, void *stream);

/* after tsidb_reset_done(done_rows, ...) and before tsidb_policy_obs, which then observes the randomised state.  Envs whose done
 * flag is set, in the sim state the reset wrote: qpos[mj_act_dof[a] + 1] += reset_joint_pos noise, qvel[mj_act_dof[a]] +=
 * reset_joint_vel noise, qvel[0:3] and qvel[3:6] += their component's noise, qpos[0:2] += reset_xy noise, qpos[2] += reset_lift,
 * and the base quaternion (wxyz) becomes (c, 0, 0, s) * quat, c = cos(t / 2), s = sin(t / 2) of t = reset_yaw (2 U - 1) formed
 * in float64 and cast - a rotation about world z - divided by its norm.  A group whose amplitude is 0 adds nothing.  The TSID
 * state q, v is left as the reset wrote it: without TSID in the loop (below) the policy environment runs no tick, and with it the
 * closed-loop tick reads the sim state itself.
 * Launches nothing and succeeds while every reset_* value is 0. */
int tsidb_policy_reset_noise(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld, void *qpos,
                             void *qvel, void *stream);

/* tsidb_policy_obs with randomisation configured (any noise amplitude, command_interval, command_zero_prob or env_offset non-zero;
 * otherwise the launch is the unrandomised kernel, bit for bit).  Commands: an env is resampled when it was not restarted,
 * command_interval > 0, ep_len > 0 and ep_len % command_interval == 0, with k = ep_len / command_interval; a restart is k = 0.
 * At either, with probability command_zero_prob (U < prob) all three components become 0; otherwise the components with
 * cmd_lo != cmd_hi are redrawn and the others stay as they are.  Noise: columns 0-2 += noise_ang_vel, 3-5 += noise_gravity,
 * 9 .. 9 + NA - 1 += noise_joint_pos, 9 + NA .. 9 + 2 NA - 1 += noise_joint_vel draws (stream 7, column = the observation column);
 * command, last action, contact flags and the privileged tail stay exact, and qpos / qvel are not touched. */

/* ---- per-episode terrain and dynamics of the policy environment, and the height scan a policy sees the ground through.  The
 * sim reads its per-env mass scale, friction, floor plane and stepped terrain from the two tables registered with
 * tsidb_set_env_params (env_params [N,8], terrain [N,20]); tsidb_policy_terrain_reset rewrites the rows of the envs a step
 * restarted, on the device, and tsidb_policy_height_scan samples the surface the sim collides against around the base.  No
 * kernel of the sim or the tick changes.  Draws are those of the randomisation above - same hash, same key layout, U in float64,
 * every value formed in float64 and cast once to the path's type - with a seed and an env_offset of their own
 * (TSIDB_POL_TER_SEED, _ENV_OFFSET: env index = env_offset + env) and streams that continue the table:
 *   stream  draw                                               column        counter
 *   12      mass scale = lo + (hi - lo) U -> env_params[0]     -             the episode about to start (episode + 1 when the kernel runs)
 *   13      friction, likewise -> env_params[1]                -             same
 *   14      tilt t = tilt_max U                                -             same
 *   15      tilt azimuth a = 2 pi U                            -             same
 *   16      strip direction g = 2 pi U                         -             same
 *   17      strip length L = lo + (hi - lo) U                  -             same
 *   18      strip c is raised iff U < step_prob                c = 0 .. 15   same
 *   19      step height H = (lo + (hi - lo) U) (lvl + 1) / num_levels   -    same
 *   20      height scan noise                                  point & 255   episode * 2^32 + ep_len (as stream 7)
 * What a restart writes, with (x_b, y_b) = qpos[0:2] of the restarted env as the reset and its noise left it:
 *   env_params = (mass scale, friction, n_x, n_y, n_z, d, 0, 0), n = (sin t cos a, sin t sin a, cos t), d = n_x x_b + n_y y_b
 *                (the plane passes through the point under the robot);
 *   terrain    = (cos g, sin g, phase, 1 / L, heights[16]), phase = (cos g) x_b + (sin g) y_b - L / 2 (cell 0 is centred under
 *                the robot), heights[c] = H where strip c is raised, else 0, and 0 for c <= flat_cells and c >= 16 - flat_cells
 *                (the start strip and flat_cells strips on each side of it; flat_cells = 0 keeps only cell 0 level).
 * lvl = level[e] clamped to 0 .. num_levels - 1, or num_levels - 1 where level is NULL: the hook of a terrain curriculum, the
 * caller's to write.  A degenerate range (lo == hi) writes that value. */
enum { TSIDB_POL_TER_SEED = 0, TSIDB_POL_TER_ENV_OFFSET, TSIDB_POL_TER_MASS_LO, TSIDB_POL_TER_MASS_HI,
       TSIDB_POL_TER_FRICTION_LO, TSIDB_POL_TER_FRICTION_HI, TSIDB_POL_TER_TILT_MAX /* rad, < pi/4 */,
       TSIDB_POL_TER_STEP_HEIGHT_LO, TSIDB_POL_TER_STEP_HEIGHT_HI /* m, >= 0 */,
       TSIDB_POL_TER_STEP_LENGTH_LO, TSIDB_POL_TER_STEP_LENGTH_HI /* m, > 0 */,
       TSIDB_POL_TER_STEP_PROB /* [0, 1] */, TSIDB_POL_TER_FLAT_CELLS /* integer 0 .. 7 */,
       TSIDB_POL_TER_NUM_LEVELS /* integer >= 1 */,
       TSIDB_POL_TER_SCAN_NX, TSIDB_POL_TER_SCAN_NY /* integers >= 0, nx * ny <= TSIDB_POL_MAXSCAN */,
       TSIDB_POL_TER_SCAN_X0, TSIDB_POL_TER_SCAN_X1, TSIDB_POL_TER_SCAN_Y0, TSIDB_POL_TER_SCAN_Y1,
       TSIDB_POL_TER_SCAN_CLIP_LO, TSIDB_POL_TER_SCAN_CLIP_HI, TSIDB_POL_TER_SCAN_NOISE, TSIDB_POL_TER_NPARAMS };
enum { TSIDB_POL_MAXSCAN = 256 };

/* Copies ter_params [TSIDB_POL_TER_NPARAMS] (host, float64) into the handle; NULL with n_params 0 switches everything off again
 * (the state of a new handle: tsidb_policy_terrain_reset fails, tsidb_policy_height_scan launches nothing).  First waits for the
 * kernels in flight, as tsidb_policy_config does.  Rejects a wrong n_params, non-finite values, any lo > hi, a mass or friction
 * lo <= 0, a tilt outside [0, pi/4), a negative height, a step length lo <= 0, a probability outside [0, 1], a non-integer where
 * an integer is named (seed, env_offset, flat_cells, num_levels, nx, ny) or one outside its range, a seed >= 2^32, an offset
 * >= 2^31, num_levels >= 2^31, nx * ny > TSIDB_POL_MAXSCAN, exactly one of nx, ny equal to 0, a negative scan_noise and
 * clip_lo > clip_hi; nothing of a rejected vector is taken. */
int tsidb_policy_terrain_config(tsidb_handle h, const double *ter_params, int n_params);

/* after tsidb_reset_done(done_rows, ...) and tsidb_policy_reset_noise, before tsidb_policy_obs.  For every env whose done flag is
 * set (column TSIDB_NOBS + 1 of done_rows [N, rows_ld >= TSIDB_NROW]) rewrites the env's row of BOTH tables registered with
 * tsidb_set_env_params as described above, from qpos [N, NQ] and level [N] (int32, device; may be NULL); the rows of the other
 * envs stay bit for bit.  A plain asynchronous launch that can be captured.  Fails (message via tsidb_last_error) while either
 * table is unregistered, before tsidb_policy_terrain_config and in a library built without the sim stage. */
int tsidb_policy_terrain_reset(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld,
                               const void *qpos, const int32_t *level, void *stream);

/* after tsidb_policy_obs.  Writes scan [N, scan_ld >= nx * ny] (the path's type; columns from nx * ny on are not touched): the
 * height of the base above the floor surface at nx * ny points of a grid that turns with the base's heading.  Point
 * p = ix * ny + iy has the offset (px, py) in the heading frame, px = x0 + (x1 - x0) ix / (nx - 1) (x0 when nx = 1), py likewise
 * from y0, y1, iy, ny, both formed in float64 and cast.  Heading h = (1 - 2 (q_y^2 + q_z^2), 2 (q_w q_z + q_x q_y)) of the base
 * quaternion qpos[3:7] (wxyz) divided by its norm, (1, 0) where |h|^2 < 1e-12: the world x, y of the base's x axis, the same
 * under any roll and pitch; no trigonometric call.  World point (X, Y) = (x_b, y_b) + (h_x px - h_y py, h_y px + h_x py), surface
 * height z_s = (d + heights[cell(X, Y) & 15] - n_x X - n_y Y) / n_z with cell = floor((direction . (X, Y) - phase) / L) of
 * tsidb_set_env_params: the surface the sim collides against (distance of x = n . x - d - heights).  The value is
 * qpos[2] - z_s clipped to [clip_lo, clip_hi] (NaN passes), then + scan_noise (2 U - 1) of stream 20 where scan_noise != 0.  An
 * unregistered table is the nominal one (n = +z, d = 0; flat), so the scan needs no randomisation.  A plain asynchronous launch
 * that can be captured; launches nothing and succeeds while nx * ny = 0. */
int tsidb_policy_height_scan(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *qpos, void *scan, int scan_ld,
                             void *stream);

/* ---- TSID in the loop of the policy environment: the policy steps the closed-loop tsidb_step (params[CLOSED_LOOP]; tick on the
 * sim state, then sim) in place of tsidb_sim_ctrl, and two more launches score it against the controller and show it the
 * controller's references.  One policy step is then tsidb_policy_act, decimation closed-loop env steps (tsidb_walk_update +
 * tsidb_step when a walking plan runs), tsidb_policy_reward, tsidb_policy_teacher, tsidb_reset_done (+ tsidb_walk_plan for the
 * done envs), tsidb_policy_obs, tsidb_policy_teacher_obs.  What ctrl means is tsidb_set_ctrl's mode: TSIDB_CTRL_RESIDUAL = the
 * policy adds a torque to TSID's tau; TSIDB_CTRL_MOTOR / _POSITION = the policy alone drives the sim and TSID is the teacher.
 * Both launches are plain asynchronous launches that can be captured.  Both fail (message via tsidb_last_error) in a library
 * built without the sim stage, while no ctrl buffer is registered, before tsidb_policy_config and before
 * tsidb_policy_teacher_config, and without the reference buffers (tsidb_set_refs).
 *
 * Teacher terms, unweighted, in the order of teacher_terms [N, TSIDB_POL_TEACH_NT] and of the weights; com, LF, RF are the
 * columns of the tick's row (tsidb_tick obs: q v com cop LF RF), com_ref / foot_ref / contact_active the registered references:
 *   track_com      exp(-|com - com_ref.pos|^2 / sigma_com^2)
 *   track_feet     exp(-(|LF - foot_ref[0].p|^2 + |RF - foot_ref[1].p|^2) / sigma_foot^2)
 *   contact_match  the number of feet (0 .. 2) whose sim contact flag c_f (tsidb_policy_reward) equals contact_active[f]
 *   deviation      sum_a ctrl_a^2 in TSIDB_CTRL_RESIDUAL mode, sum_a (ctrl_a - tau[mj_ctrl_qidx[a] - 7])^2 in TSIDB_CTRL_MOTOR mode
 *                  (tau in the actuator order), 0 in TSIDB_CTRL_POSITION mode */
enum { TSIDB_POL_TEACH_NT = 4, TSIDB_POL_TEACH_NOBS = 34 /* 14 + NA: the v1 robot's; 32 for robot/v0 */ };

/* tsidb_policy_teacher_config's parameter vector (float64, host) */
enum {
  TSIDB_POL_TEACH_SIGMA_COM = 0 /* m, > 0 */, TSIDB_POL_TEACH_SIGMA_FOOT /* m, > 0 */, TSIDB_POL_TEACH_WEIGHTS /*TSIDB_POL_TEACH_NT*/,
  TSIDB_POL_TEACH_NPARAMS = TSIDB_POL_TEACH_WEIGHTS + TSIDB_POL_TEACH_NT
};

/* Copies teach_params [TSIDB_POL_TEACH_NPARAMS] into the handle; first waits for the kernels in flight, as tsidb_policy_config
 * does.  Rejects a wrong n_params, non-finite values and a sigma <= 0; nothing of a rejected vector is taken. */
int tsidb_policy_teacher_config(tsidb_handle h, const double *teach_params, int n_params);

/* after tsidb_policy_reward, before tsidb_reset_done.  rows [N, rows_ld >= TSIDB_NROW] as the last tick of tsidb_step wrote them,
 * with reward and done in columns TSIDB_NOBS and TSIDB_NOBS + 1 as tsidb_policy_reward left them; q [N, NQ] the TSID state that
 * tick ended on, tau [N, NA] and status [N] its outputs, ncon / con_pairs the last sim step's.  Writes teacher_terms and
 * reward += sum_k weights[k] teacher_terms[k].  An env whose status != 0 (TSID's QP failed) becomes terminated: done = 1,
 * timeout = 0, the termination term of tsidb_policy_bufs.terms set to 1, and reward += the termination weight of
 * tsidb_policy_config unless tsidb_policy_reward had terminated the env already.  Writes teacher_action [N, NA], the action
 * that reproduces TSID's command through tsidb_policy_act's map (no delay, no filter), clipped to +-clip and 0 where
 * scale[a] = 0: (tau[mj_ctrl_qidx[a] - 7] - default[a]) / scale[a] in TSIDB_CTRL_MOTOR mode, (q[mj_ctrl_qidx[a]] - default[a]) /
 * scale[a] in TSIDB_CTRL_POSITION mode, 0 in TSIDB_CTRL_RESIDUAL mode.  All of this launch's arithmetic runs in float64 on the
 * path's buffers, with scale, default, clip and the weights as the two config calls were given them, and is cast once when it is
 * stored - as the randomisation forms its draws. */
int tsidb_policy_teacher(tsidb_handle h, const tsidb_policy_bufs *bufs, void *rows, int rows_ld, const void *q, const void *tau,
                         const int32_t *status, const int32_t *ncon, const int32_t *con_pairs, void *teacher_terms,
                         void *teacher_action, void *stream);

/* after tsidb_policy_obs.  Writes teacher_obs [N, obs_ld >= 14 + NA]; R is the rotation of the sim base (qpos, wxyz), so R^T v
 * is v in the base frame, as the observation's velocities:
 *   0-1 contact_active of the two feet   2-4 R^T (com_ref.pos - com)   5-7 R^T com_ref.vel   8-10 R^T (foot_ref[0].p - LF)
 *   11-13 R^T (foot_ref[1].p - RF)   14.. TSID's tau in the actuator order (NA: tau[mj_ctrl_qidx[a] - 7])
 * For an env the step just restarted (done flag in column TSIDB_NOBS + 1 of rows) the three error groups and tau are 0 - the
 * tick's row is the fallen robot's, and a reset robot stands on its references - while contact_active and com_ref.vel are what
 * the reset wrote.  No noise is ever added to these columns. */
int tsidb_policy_teacher_obs(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *rows, int rows_ld, const void *qpos,
                             const void *tau, void *teacher_obs, int obs_ld, void *stream);

/* ---- imitation of the teacher: the label of a stored rollout row and DAgger's mixing.  After tsidb_policy_actor (which stored the
 * row and sampled `action`), before tsidb_policy_act.  One plain asynchronous launch: no allocation, no host read, capturable.
 * teacher_action [N, NA] (the path's type) is what tsidb_policy_teacher wrote at the end of the PREVIOUS policy step.  Timing: it
 * was formed by the last tick of that step, on the state one sim step before the observation the actor has just seen - the
 * closest label the closed loop offers, and a causal one: the same tau is in teacher_obs.  For an env the previous step restarted,
 * or tsidb_reset / PolicyEnv.reset() has just set up, it belongs to the fallen robot or to nothing: that is ep_len == 0, and such
 * a row gets weight 0 and is never executed (a failed QP ends in a restart, so it is covered too).  Per env e:
 *   label[e, a]  = (float)teacher_action[e, a]                 cast once; label [N, NA] float32
 *   weight[e]    = ep_len[e] > 0 ? 1 : 0                       [N] float32
 *   executed[e]  = U < beta[0] && ep_len[e] > 0                [N] int32
 *   action[e, :] = teacher_action[e, :] where executed[e]      the path's bits, an exact copy; elsewhere action keeps its bits
 * with U one more stream of the randomisation's key layout (key = seed + ((stream * 256 + column) * 2^32), the same hash):
 *   stream  draw                     column              counter
 *   23      teacher / student episode  -                 episode * 2^32: one draw per episode - a whole episode is the teacher's
 *                                                        or the student's
 * for the env index env_offset + env; episode and ep_len are read from bufs.  beta [1] float32 is read from DEVICE memory at
 * every launch (as tsidb_policy_opt_step reads lr): a captured rollout follows a beta that a device op decays between replays;
 * NULL = 0, nothing is executed.  action may be NULL (labels and flags alone).  Rejects (message via tsidb_last_error, nothing
 * launched): what tsidb_policy_act rejects in bufs and the handle's state; a NULL teacher_action, label, weight or executed;
 * seed >= 2^32; env_offset >= 2^31. */
int tsidb_policy_teacher_mix(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *teacher_action, void *action, float *label,
                             float *weight, int32_t *executed, const float *beta, uint64_t seed, uint64_t env_offset, void *stream);

/* ---- episode statistics and a terrain curriculum: what a training loop logs every iteration (mean episode return and length,
 * per-term episode sums, share of timeouts, distance travelled) and legged_gym's terrain curriculum (_update_terrain_curriculum),
 * kept on the device inside the step - tsidb_policy_episode_end after tsidb_policy_reward (and tsidb_policy_teacher where it runs)
 * and before tsidb_reset_done, which wipes the final position of a fallen env; tsidb_policy_episode_begin after tsidb_reset_done,
 * tsidb_policy_reset_noise and tsidb_policy_terrain_reset, where the first position of the new episode exists.  Off by default:
 * neither launch is made by anything else, and no other entry reads what they write except tsidb_policy_terrain_reset its level.
 *
 * The record of an episode, float64 whatever the path's type (as the normaliser's statistics), TSIDB_POL_EP_NREC columns:
 *   COUNT         1 per finished episode
 *   TIMEOUT       1 if the episode ended by its length alone (timeout of tsidb_policy_bufs)
 *   LENGTH        policy steps: ep_len after tsidb_policy_reward incremented it
 *   RETURN        sum over the episode of the env's reward as it stands in the rows when the kernel runs, teacher terms included
 *   DISPLACEMENT  d = sqrt(dx^2 + dy^2) of the base xy between the episode's first state and its last [m]
 *   LEVEL         the terrain level the episode ran on
 *   TERMS ..      the TSIDB_POL_NT sums of the unweighted reward terms
 *   TEACH ..      the TSIDB_POL_TEACH_NT sums of the unweighted teacher terms; 0 while no teacher_terms pointer is given */
enum { TSIDB_POL_EP_COUNT = 0, TSIDB_POL_EP_TIMEOUT, TSIDB_POL_EP_LENGTH, TSIDB_POL_EP_RETURN, TSIDB_POL_EP_DISPLACEMENT, TSIDB_POL_EP_LEVEL,
       TSIDB_POL_EP_TERMS /*TSIDB_POL_NT*/, TSIDB_POL_EP_TEACH = TSIDB_POL_EP_TERMS + TSIDB_POL_NT /*TSIDB_POL_TEACH_NT*/,
       TSIDB_POL_EP_NREC = TSIDB_POL_EP_TEACH + TSIDB_POL_TEACH_NT };

/* tsidb_policy_episode_config's parameter vector (float64, host) */
enum { TSIDB_POL_EPP_CURRICULUM = 0 /* 0 / 1: tsidb_policy_episode_end writes level */, TSIDB_POL_EPP_UP_DISTANCE /* m, > 0 */,
       TSIDB_POL_EPP_DOWN_FRACTION /* >= 0, of the distance the command asked for */, TSIDB_POL_EPP_RANDOM_TOP /* 0 / 1 */,
       TSIDB_POL_EPP_NPARAMS };

/* the per-env episode state: device buffers owned by the caller; all but level and teacher_terms are required */
typedef struct tsidb_policy_episode {
  double *run;               /* [N, TSIDB_POL_EP_NREC] the running episode's sums in the columns LENGTH, RETURN, TERMS, TEACH; the others stay 0 */
  double *start_xy;          /* [N, 2] base xy of the running episode's first state */
  double *last;              /* [N, TSIDB_POL_EP_NREC] the record of the env's most recently finished episode */
  double *sum;               /* [N, TSIDB_POL_EP_NREC] per-env sums of the records since the caller last zeroed it */
  int32_t *level;            /* [N] the terrain level tsidb_policy_terrain_reset reads; may be NULL while the curriculum is off */
  const void *teacher_terms; /* [N, TSIDB_POL_TEACH_NT] in the path's type, as tsidb_policy_teacher wrote them; may be NULL */
} tsidb_policy_episode;

/* Copies ep_params [TSIDB_POL_EPP_NPARAMS] (host, float64) into the handle; NULL with n_params 0 switches the slice off again (the
 * state of a new handle: both launches fail).  First waits for the kernels in flight, as tsidb_policy_config does.  Rejects a
 * wrong n_params, non-finite values, a flag other than 0 / 1, UP_DISTANCE <= 0 with the curriculum on and a negative fraction;
 * nothing of a rejected vector is taken.  The curriculum also needs tsidb_policy_terrain_config (num_levels, the seed and the env
 * offset are the terrain's), max_episode_steps > 0 and a level pointer: tsidb_policy_episode_end fails without them. */
int tsidb_policy_episode_config(tsidb_handle h, const double *ep_params, int n_params);

/* after tsidb_policy_reward (and tsidb_policy_teacher), before tsidb_reset_done.  qpos [N, NQ] the sim state the step ended on;
 * reward and done point at the first env's values, row_ld elements apart, as tsidb_policy_reward takes them; terms, timeout,
 * ep_len, episode and command are read from bufs.  For every env, with x+ = x finite ? x : 0 (a select: one NaN step does not
 * poison an iteration's log):
 *   run[LENGTH] += 1, run[RETURN] += (double)reward +, run[TERMS + k] += (double)terms[k] +, run[TEACH + k] += (double)teacher_terms[k] +
 * For an env whose done flag is set: record = (1, timeout, ep_len, run[RETURN], d, lvl, run[TERMS ..], run[TEACH ..]) with
 * d = |(double)qpos[0:2] - start_xy| and lvl = level[e] clamped to 0 .. num_levels - 1 (to >= 0 before
 * tsidb_policy_terrain_config; 0 where level is NULL); last[e] = record; sum[e] += record, RETURN and DISPLACEMENT through the
 * same select.  last of the other envs is not touched.
 * With the curriculum on, level[e] of a done env becomes legged_gym's rule, L = num_levels, T = max_episode_steps * (decimation *
 * dt) - the seconds of a whole episode, decimation * dt the step tsidb_policy_reward advances the air times by:
 *   up = d > UP_DISTANCE;  down = !up && d < DOWN_FRACTION |command_xy| T  (the command as it stands, before the reset redraws it)
 *   lvl += up - down;  below 0 -> 0;  >= L -> RANDOM_TOP ? min(L - 1, floor(U L)) : L - 1
 * everything in float64; a NaN d compares false both ways and leaves the clamped level.  U is one more stream of the
 * randomisation's key layout (key = seed + ((stream * 256 + column) * 2^32), the same hash), seed and env_offset the terrain's:
 *   stream  draw                     column              counter
 *   24      graduate's level         -                   the episode about to start (episode + 1 when the kernel runs), as 12-19
 * A plain asynchronous launch in the policy kernels' shape: no atomics, no host read, no allocation, capturable.  Fails (message
 * via tsidb_last_error) where tsidb_policy_act fails, before tsidb_policy_episode_config, on a NULL required buffer or
 * row_ld < 1, and with the curriculum on before tsidb_policy_terrain_config, with max_episode_steps = 0 or with level NULL. */
int tsidb_policy_episode_end(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_episode *ep, const void *qpos,
                             const void *reward, const void *done, int row_ld, void *stream);

/* after tsidb_reset_done(done_rows, ...), tsidb_policy_reset_noise and tsidb_policy_terrain_reset; before or after
 * tsidb_policy_obs.  For an env whose done flag is set (column TSIDB_NOBS + 1 of done_rows [N, rows_ld >= TSIDB_NROW]):
 * start_xy = (double)qpos[0:2] and the run row zeroed; every other row stays bit for bit.  Launch and failures as above (the
 * curriculum asks nothing of this one). */
int tsidb_policy_episode_begin(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_episode *ep, const void *done_rows,
                               int rows_ld, const void *qpos, void *stream);

/* ---- observation history: the last `frames` observations of every env stacked into one row, what a feed-forward actor is given
 * in place of a memory (Isaac Lab's history_length, the frame stacks of legged_gym and humanoid-gym).  One launch per policy step,
 * behind the kernels that write the observation tensors; nothing else reads or writes the history.
 *
 * A frame is the concatenation of 1 .. TSIDB_POL_OBSH_MAXSRC column blocks of the caller's tensors, src[i][e * src_ld[i] + c] for
 * c < src_cols[i], in the path's type and in the order given (any [N, k] view with a row stride: obs or priv inside their row, a
 * column range of either, command, the height scan, the teacher's observation; the same tensor may be named twice); K = the sum
 * of src_cols.  history [N, frames * K] in the path's type is frame-major, oldest frame first: frame f of env e is
 * history[e * frames * K + f * K + k], k < K, and the newest frame, f = frames - 1, is the row an actor without a history
 * would see.  frames * K <= TSIDB_POL_OBSH_MAXCOLS.  Frames are copies: what the observation kernels left in the sources,
 * observation noise included, bit for bit. */
enum { TSIDB_POL_OBSH_MAXSRC = 4, TSIDB_POL_OBSH_MAXFRAMES = 32, TSIDB_POL_OBSH_MAXCOLS = 4096 };

/* device buffers owned by the caller.  THE SOURCES AND history MUST NOT OVERLAP: the library cannot check it.  The struct shares
 * its name with the entry point, as stat does: it has no typedef and is always written `struct tsidb_policy_obs_history`. */
struct tsidb_policy_obs_history {
  void *history;                             /* [N, frames * K] */
  int frames;                                /* 1 .. TSIDB_POL_OBSH_MAXFRAMES */
  int n_src;                                 /* 1 .. TSIDB_POL_OBSH_MAXSRC */
  const void *src[TSIDB_POL_OBSH_MAXSRC];    /* first column of each block, env 0 */
  int src_ld[TSIDB_POL_OBSH_MAXSRC];         /* row stride in elements, >= src_cols */
  int src_cols[TSIDB_POL_OBSH_MAXSRC];       /* columns of each block, >= 1 */
};

/* after tsidb_reset_done(done_rows, ...) and the launches that write the sources (tsidb_policy_obs, tsidb_policy_height_scan,
 * tsidb_policy_teacher_obs).  With x[e] the current frame of env e:
 *   done flag set (column TSIDB_NOBS + 1 of done_rows [N, rows_ld >= TSIDB_NROW]): every one of the `frames` frames = x[e] -
 *     the first observation of an episode carries nothing of the one that ended;
 *   otherwise, push = 1 (a policy step): frame[f] = frame[f + 1] for f < frames - 1, frame[frames - 1] = x[e];
 *   otherwise, push = 0 (a reset of other envs, which recomputes the observations but is no new time step): untouched, bit for bit.
 * So the newest frame always equals the current selection.  The shift is in place; the struct is copied into the launch and the
 * handle keeps nothing of it.  A plain asynchronous launch in the policy kernels' shape: no atomics, no host read, no
 * allocation, capturable.  Fails (message via tsidb_last_error) on a NULL struct, history or source, frames or n_src out of
 * range, src_cols < 1, src_ld < src_cols, frames * K > TSIDB_POL_OBSH_MAXCOLS, done_rows NULL or rows_ld < TSIDB_NROW, and a
 * push other than 0 / 1. */
int tsidb_policy_obs_history(tsidb_handle h, const struct tsidb_policy_obs_history *hist, const void *done_rows, int rows_ld,
                             int push, void *stream);

/* ---- the policy's side of a rollout: a dense actor and an optional critic evaluated on the env's own rows, the Gaussian sample
 * with its log-probability, and the advantages of a recorded rollout.  Both calls are plain asynchronous launches on the given
 * stream: no allocation, no host synchronisation, no state of their own - T policy steps with their actor calls can be captured
 * as one graph.  Hot path: f32-input MFMA (v_mfma_f32_16x16x4_f32), exact float32 products and sums whatever the path's type.
 *
 * A network is 1 .. TSIDB_POL_NET_MAXLAYERS dense layers, y = weight x + bias, each at most TSIDB_POL_NET_MAXWIDTH wide, with
 * the hidden activation after every layer but the last (ELU with alpha = 1, tanh or ReLU); the last layer is linear.  weight
 * [width, fan-in] row-major and bias [width] (NULL = none) are float32 device pointers in torch.nn.Linear's own layout, READ IN
 * PLACE AT EVERY LAUNCH: nothing is packed or cached, so an optimiser step on the tensors behind them is seen by the next launch.
 * The input row of env e is the concatenation of 1 .. TSIDB_POL_NET_MAXBLOCKS column blocks, block[i][e * block_ld[i] + c] for
 * c < block_cols[i], in the path's type (cast to float32 on load; any [N, k] view with a row stride, such as obs inside its
 * TSIDB_POL_NOBS + TSIDB_POL_NPRIV row); at most TSIDB_POL_NET_MAXWIDTH columns in total = the fan-in of layer 0.  The struct is
 * copied into the launch; the handle keeps nothing of it. */
enum { TSIDB_POL_NET_MAXLAYERS = 4, TSIDB_POL_NET_MAXBLOCKS = 4, TSIDB_POL_NET_MAXWIDTH = 512 };
enum { TSIDB_POL_ACT_ELU = 0, TSIDB_POL_ACT_TANH = 1, TSIDB_POL_ACT_RELU = 2 };
enum { TSIDB_POL_ACTOR_SAMPLE = 1 /* flags bit 0 */ };
typedef struct tsidb_policy_net {
  int n_layers;
  int width[4];           /* outputs of each layer */
  int activation;         /* TSIDB_POL_ACT_* */
  const float *weight[4];
  const float *bias[4];
  int n_blocks;
  const void *block[4];
  int block_ld[4];        /* row stride in elements, >= block_cols */
  int block_cols[4];
} tsidb_policy_net;

/* what tsidb_policy_actor writes; every pointer is optional (NULL = not written), rows at or beyond N are never touched */
typedef struct tsidb_policy_actor_out {
  void *action;           /* [N, NA] the path's type: action32 cast, ready for tsidb_policy_act */
  float *action32;        /* [N, NA] */
  float *mean;            /* [N, NA] the actor's output */
  float *logp;            /* [N] */
  float *value;           /* [N] the critic's output */
  float *actor_input;     /* [N, K_actor] the assembled float32 input rows */
  float *critic_input;    /* [N, K_critic] */
} tsidb_policy_actor_out;

/* Evaluates the actor (last width = NA) and, unless critic is NULL, the critic (last width = 1) for every env, in one launch; actor
 * may be NULL in a call with a critic (the value alone: the last row of a rollout, no draw whatever the flags).  flags bit 0
 * (TSIDB_POL_ACTOR_SAMPLE) clear: action = mean, no draw.  Set: log_std [NA] float32 (device, read in place) and
 *   eps_a = sqrt(-2 ln(1 - U1)) cos(2 pi U2), formed in float64 and cast to float32 once;   action_a = mean_a + exp(log_std_a) eps_a
 * with U1, U2 two more streams of the randomisation's key layout (key = seed + ((stream * 256 + column) * 2^32), the same hash):
 *   stream  draw                     column              counter
 *   21      action noise, U1         actuator            episode * 2^32 + ep_len, as the observation noise (stream 7)
 *   22      action noise, U2         actuator            same
 * for the env index env_offset + env; episode and ep_len are read from bufs.  TWO CALLS ON THE SAME (env, episode, ep_len) DRAW
 * THE SAME NOISE: the sample belongs to the observation, not to the call, and a batch split over ranks draws what the unsplit
 * batch draws.  logp = -sum_a (eps_a^2 / 2 + log_std_a) - NA ln(2 pi) / 2, the log-probability of the unclipped sample (eps = 0
 * without the flag; log_std = 0 where it is NULL); the clip stays tsidb_policy_act's.  bufs may be NULL without the flag.
 * Rejects (message via tsidb_last_error, nothing launched): a NULL out, both networks NULL, n_layers outside 1 .. 4, n_blocks outside
 * 1 .. 4, a width or an input total of 0 or above 512, block_cols < 1, block_ld < block_cols, a NULL block or weight, an unknown
 * activation, an actor whose last width is not NA, a critic whose last width is not 1, the flag without bufs (episode, ep_len)
 * or log_std, a seed >= 2^32 or an env_offset >= 2^31. */
int tsidb_policy_actor(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                       const tsidb_policy_actor_out *out, const void *log_std, uint64_t seed, uint64_t env_offset, int flags,
                       void *stream);

/* ---- observation normalisation: rsl_rl's EmpiricalNormalization (empirical_normalization = True) on the policy's input rows,
 * one state per network over the K columns of its assembled row, applied by the actor's own launch as it loads the blocks.
 *   stats  [2, K] float64   running mean, running variance        initial 0, 1
 *   count  [1]    int64     rows seen                              initial 0
 *   affine [2, K] float32   shift = (float)mean, scale = (float)(1 / (sqrt(var) + eps))  - all the actor reads
 * (device memory the caller owns; eps > 0, rsl_rl's default 1e-2; the map is rsl_rl's (x - mean) / (std + eps)).
 *
 * tsidb_policy_norm_update folds the N current rows into the state of each network given.  Everything is float64 on
 * x = (double)(float)block[i][e * block_ld[i] + c], the value the actor sees, not the float64 original:
 *   mean_b, var_b = mean and BIASED variance of the N rows of a column, two passes (the mean, then the centred squares)
 *   count' = count + N;  rate = N / count'
 *   delta = mean_b - mean;  mean' = mean + rate * delta
 *   var'  = var + rate * (var_b - var + delta * (mean_b - mean'))
 * then affine is rewritten from (mean', var').  until > 0: when count >= until - read FROM DEVICE MEMORY by the kernel, there
 * is no host read - the call changes nothing, so count stops at the first value >= until.  0 = no limit.
 * ORDER AND DETERMINISM: the rows are cut into segments of TSIDB_POL_NORM_SEG_ROWS whatever the device; within a segment a
 * column's rows r are summed per residue r mod 16 in rising r, the 16 sums then in rising residue, for the mean and again for
 * the centred squares; the segments' (n, mean, M2) are merged in segment order by Chan's formula
 *   d = mean_s - mean;  mean += d n_s / (n + n_s);  M2 += M2_s + d^2 n n_s / (n + n_s)
 * by one lane per column.  No atomics, no bit depends on the grid: two calls from the same state write the same bits (a
 * permutation of the envs may change them).  Two plain asynchronous launches on the given stream, both networks in each (grid
 * axis = network): no allocation, no host synchronisation, capturable in a graph.
 * workspace: device memory of tsidb_policy_norm_workspace's bytes - 16 * ceil(N / SEG_ROWS) * (K_actor + K_critic) - rewritten
 * by every call.  The networks are tsidb_policy_net as tsidb_policy_actor takes them; only the block fields are read, rows at or
 * beyond N never.  Either network may be NULL (its norm is then ignored).
 * Rejects (message via tsidb_last_error, nothing launched): both networks NULL; a network whose norm is NULL or has a NULL
 * stats, count or affine; eps <= 0 or not finite; until < 0; a NULL workspace or one smaller than the query's; n_blocks outside
 * 1 .. 4, block_cols < 1, block_ld < block_cols, a NULL block, an input total above 512 - what tsidb_policy_actor rejects in a
 * network's block fields.
 *
 * tsidb_policy_actor_norm is tsidb_policy_actor with the map applied on load: for a network whose norm is given (non-NULL, with
 * a non-NULL affine) column c of the row becomes
 *   v = ((float)x - shift[c]) * scale[c]     one float32 subtraction, one float32 product, no fused multiply-add
 *   v = min(max(v, -clip), clip)             where clip > 0 (0 = none)
 * and THIS v is what the layers see and what actor_input / critic_input receive: a rollout stores the normalised rows, as
 * rsl_rl does, and tsidb_policy_learn recomputes the actor's outputs from them bit for bit without knowing of the normaliser.
 * It reads affine and clip only; stats, count, eps and until are the update's.  With both norms NULL (or their affine NULL) it IS
 * tsidb_policy_actor: the same kernel, the same bits.  tsidb_policy_net is unchanged, so tsidb_policy_learn and its workspace
 * query cannot see a normaliser.  Rejects what tsidb_policy_actor rejects, a norm for a NULL network, and clip < 0 or NaN.
 * Not done here: a non-finite input poisons the statistics, as in rsl_rl (no masking); the statistics are per process - a batch
 * split over ranks is not split-invariant, a rank merge belongs with an all-reduce. */
enum { TSIDB_POL_NORM_SEG_ROWS = 256 };
typedef struct tsidb_policy_norm {
  float *affine;          /* [2, K] float32: shift, scale */
  float clip;             /* 0 = none */
  double *stats;          /* [2, K] float64: mean, variance */
  int64_t *count;         /* [1] */
  double eps;
  int64_t until;          /* 0 = no limit */
} tsidb_policy_norm;

int tsidb_policy_norm_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, size_t *bytes);

int tsidb_policy_norm_update(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                             const tsidb_policy_norm *actor_norm, const tsidb_policy_norm *critic_norm, void *workspace,
                             size_t workspace_bytes, void *stream);

int tsidb_policy_actor_norm(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                            const tsidb_policy_norm *actor_norm, const tsidb_policy_norm *critic_norm,
                            const tsidb_policy_actor_out *out, const void *log_std, uint64_t seed, uint64_t env_offset, int flags,
                            void *stream);

/* Generalised advantage estimation over T recorded policy steps, float32, one lane per env, backwards from A_T = 0:
 *   r'_t = r_t + gamma V_t timeout_t;   delta_t = r'_t + gamma V_{t+1} (1 - done_t) - V_t;
 *   A_t = delta_t + gamma lam (1 - done_t) A_{t+1};   returns_t = A_t + V_t
 * reward, done [T, N] in the path's type, timeout [T, N] int32, value [T + 1, N] float32 (the last row: the critic on the
 * observation after the last step); advantage, returns [T, N] float32.  Rejects T < 1 and a NULL buffer. */
int tsidb_policy_gae(tsidb_handle h, int T, const void *reward, const void *done, const int32_t *timeout, const float *value,
                     float gamma, float lam, float *advantage, float *returns, void *stream);

/* ---- the update's side of a PPO iteration: the loss of one minibatch of stored rollout rows and its gradient with respect to
 * every weight and bias of the actor and the critic and to log_std.  The optimiser, gradient clipping and schedules stay the
 * caller's unless PolicyOptimizer is used (tsidb_policy_opt_step below), all-reduces stay the caller's, on the gradient buffers.  Plain asynchronous launches on the given stream (three kernels): no allocation, no
 * host synchronisation, capturable in a graph.  Hot path: v_mfma_f32_16x16x4_f32, float32 throughout.  NO ATOMICS: every sum has
 * one fixed order, the rows are cut into segments of TSIDB_POL_LEARN_SEG_ROWS whatever the device, so two calls on the same
 * inputs write the same bits.
 *
 * The networks are tsidb_policy_net as tsidb_policy_actor takes them, weights and biases READ IN PLACE; the forward pass is
 * k_policy_actor's own, bit for bit.  Of the block fields only n_blocks and block_cols are read - their total is the fan-in K of
 * layer 0 - the input rows come from the batch: minibatch row m is the stored row j = index[m] of
 *   actor_input [rows, K_actor], critic_input [rows, K_critic], action [rows, NA], logp, value, advantage, returns [rows]
 * (float32, contiguous: a rollout's [T, N, ...] tensors with rows = T * N; value may be longer).  adv_stats [2] float32 (device):
 * mean and 1 / std of the advantage, NULL = not normalised.  With c = clip, sigma = exp(log_std), per row:
 *   mu = actor(actor_input[j]);  z = (action[j] - mu) / sigma;  logp = -sum_a (z_a^2 / 2 + log_std_a) - NA ln(2 pi) / 2
 *   r = exp(logp - logp_old[j]);  Ahat = (advantage[j] - adv_stats[0]) * adv_stats[1]
 *   L_pi = mean_m max(-Ahat r, -Ahat clamp(r, 1 - c, 1 + c))
 *   v = critic(critic_input[j]);  v_clip = value[j] + clamp(v - value[j], -c, c)
 *   L_v = mean_m max((v - returns[j])^2, (v_clip - returns[j])^2)      (value_clip = 0: (v - returns[j])^2)
 *   entropy = sum_a (log_std_a + (1 + ln 2 pi) / 2);   loss = L_pi + value_coef L_v - entropy_coef entropy
 * and the gradient is torch.autograd's for these expressions, ties included (a max of two equal terms gives each half).
 * Written, OVERWRITTEN not accumulated: actor_grads / critic_grads (weight[l] [width, fan-in], bias[l] [width]; a bias gradient
 * is required where the network has the bias), log_std_grad [NA], and stats [8] float32:
 *   0 L_pi   1 L_v   2 entropy   3 mean (logp_old - logp)   4 fraction of rows with r outside [1 - c, 1 + c]   5 loss
 *   6 rows used   7 bad indices
 * A row whose index is outside [0, rows) is not read, contributes nothing and is counted in stats[7]; the means stay over M.
 * critic may be NULL (critic_grads unused, L_v = 0).
 *
 * workspace: float32 device memory of at least tsidb_policy_learn_workspace's bytes (a function of the two networks and M),
 * rewritten by every call.  With Mp = M rounded up to a multiple of 16 its first Mp * NA floats are mu [Mp, NA] and the next Mp
 * floats v (with a critic), as the forward pass computed them for the M rows; the rest is the library's.
 * Rejects (message via tsidb_last_error, nothing launched): a NULL actor, batch, actor_grads, cfg, log_std, log_std_grad, stats,
 * workspace, index or stored array the call reads; critic_grads NULL with a critic; everything tsidb_policy_actor rejects in a
 * network apart from its block pointers and strides; a NULL weight gradient, a NULL bias gradient where the bias exists; M < 1,
 * rows < 1; a workspace smaller than the query's; clip <= 0; a critic without critic_input, value or returns. */
enum { TSIDB_POL_LEARN_SEG_ROWS = 512, TSIDB_POL_LEARN_NSTATS = 8 };
typedef struct tsidb_policy_learn_batch {
  const float *actor_input;
  const float *critic_input;
  const float *action;
  const float *logp;
  const float *value;
  const float *advantage;
  const float *returns;
  const int32_t *index;      /* [M] device */
  int rows;
  int M;
  const float *adv_stats;
} tsidb_policy_learn_batch;

typedef struct tsidb_policy_grads {
  float *weight[4];
  float *bias[4];
} tsidb_policy_grads;

typedef struct tsidb_policy_learn_cfg {
  float clip;
  float value_coef;
  float entropy_coef;
  int value_clip;
} tsidb_policy_learn_cfg;

int tsidb_policy_learn_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes);

int tsidb_policy_learn(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                       const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                       const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                       const tsidb_policy_learn_cfg *cfg, float *workspace, size_t workspace_bytes, float *stats, void *stream);

/* tsidb_policy_learn with an imitation term on the actor's mean (rsl_rl's Distillation; PPO with a behaviour-cloning term) and a
 * weight on the surrogate.  Everything above holds - three launches, no atomics, one fixed order of every sum, the workspace's
 * first floats mu and v - with these additions.  Per minibatch row m with j = index[m] valid, d_a = mu_a - target[j, a],
 * w = weight[j] (1 where weight is NULL):
 *   TSIDB_POL_IMIT_MSE     l_m = (1 / NA) sum_a d_a^2
 *   TSIDB_POL_IMIT_HUBER   l_m = (1 / NA) sum_a (|d_a| <= 1 ? d_a^2 / 2 : |d_a| - 1/2)        (delta = 1, torch's default)
 *   L_im = (1 / M) sum_m w l_m
 *   loss = surrogate_coef L_pi + value_coef L_v - entropy_coef entropy + imitation_coef L_im
 * The gradient is torch.autograd's for these expressions: dmu_a gains imitation_coef w / (M NA) times 2 d_a (MSE) or
 * clamp(d_a, -1, 1) (Huber); log_std gets nothing from the term (the label is for the mean, as in rsl_rl's act_inference); the
 * surrogate's dlogp, and with it its share of dlog_std, is scaled by surrogate_coef.  surrogate_coef = 1: PPO as it is;
 * surrogate_coef = value_coef = entropy_coef = 0: pure distillation.
 * A row with w == 0 exactly contributes exactly 0 and its target is NOT READ (a select, not a product: a NaN label behind a zero
 * weight is harmless).  A row whose skip_surrogate[j] is nonzero - the env executed another action than the stored one
 * (tsidb_policy_teacher_mix) - contributes 0 to L_pi, to dlogp and to stats[3] and stats[4]; its value loss and its imitation term
 * stay, and it still counts in stats[6].  All means stay over M; a bad index contributes nothing to the new term either.
 * stats[0..7] keep their meanings, stats[5] is the full loss above.  imit->stats [TSIDB_POL_IMIT_NSTATS] float32:
 *   0 L_im (formed wherever target is given, also with imitation_coef = 0)   1 sum of w over the rows used
 *   2 rows used with w > 0   3 rows used whose surrogate was skipped
 * With imitation_coef = 0 the labels add nothing to any gradient or to stats[5] whatever they hold; with surrogate_coef = 1 and
 * no skipped row besides, the gradients and stats[0..7] are tsidb_policy_learn's bit for bit.  imit NULL is tsidb_policy_learn:
 * the same kernels, the same bits, tsidb_policy_learn_workspace's bytes.  Otherwise the workspace is at least
 * tsidb_policy_learn_imit_workspace's bytes (four more floats per row and per segment than tsidb_policy_learn_workspace).
 * Rejects: what tsidb_policy_learn rejects; a NULL target with imitation_coef > 0; a NULL imit->stats; a negative or non-finite
 * imitation_coef, surrogate_coef, value_coef or entropy_coef; an unknown loss.
 * (The struct is tsidb_policy_imit: C has one namespace for a typedef and a function, so it cannot share the entry's name.) */
enum { TSIDB_POL_IMIT_MSE = 0, TSIDB_POL_IMIT_HUBER = 1 };
enum { TSIDB_POL_IMIT_NSTATS = 4 };
typedef struct tsidb_policy_imit {
  const float *target;            /* [rows, NA] the stored labels */
  const float *weight;            /* [rows] >= 0, NULL = 1 */
  const int32_t *skip_surrogate;  /* [rows], NULL = none: nonzero = the row was not the policy's action */
  float imitation_coef;           /* >= 0 */
  float surrogate_coef;           /* >= 0 */
  int loss;                       /* TSIDB_POL_IMIT_* */
  float *stats;                   /* [TSIDB_POL_IMIT_NSTATS] */
} tsidb_policy_imit;

int tsidb_policy_learn_imit_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes);

int tsidb_policy_learn_imit(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                            const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                            const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                            const tsidb_policy_learn_cfg *cfg, const tsidb_policy_imit *imit, float *workspace,
                            size_t workspace_bytes, float *stats, void *stream);

/* tsidb_policy_learn with the robot's left / right symmetry (rsl_rl's symmetry_cfg: use_data_augmentation, use_mirror_loss,
 * mirror_loss_coeff).  Everything of tsidb_policy_learn holds - three launches, no atomics, one fixed order of every sum, no
 * host read, no allocation, capturable - with these additions.  A mirror map is a signed permutation of a row,
 * mirror(x)[c] = sign[c] * x[perm[c]]: S_o of the actor's input row (actor_perm, actor_sign [K_actor]), S_c of the critic's
 * (critic_perm, critic_sign [K_critic]; unused without a critic), S_a of the action (action_perm, action_sign [NA]); int32 and
 * float32 device arrays.  A perm entry outside its row makes that mirrored column 0; nothing is read out of bounds.
 * For minibatch row m with j = index[m] valid: x' = S_o x, a' = S_a action[j]; logp_old, value, advantage and returns of the
 * mirrored row are its original's.
 *   augment != 0: L_pi, L_v, stats[3], stats[4] are means over the 2 M virtual rows (the M originals and their M mirrors, each
 *     weighted 1 / (2 M)), the critic sees S_c of its own input, dlog_std sums over the 2 M rows, stats[6] counts the virtual rows
 *     used, stats[7] counts each bad index once.
 *   L_sym = 1 / (M NA) sum_m | mu(x'_m) - S_a mu(x_m) |^2;   loss = (the above) + mirror_coef L_sym.  The target S_a mu(x_m) is
 *     a constant: the gradient flows through mu(x'_m) alone (dmu' gains mirror_coef 2 d / (M NA)); log_std gets nothing from it.
 *   augment == 0: the mirrored rows carry the mirror term alone - no mirrored rows for the critic, the means stay over M.
 * sym->stats [TSIDB_POL_SYM_NSTATS] float32: 0 L_sym (formed at mirror_coef = 0 too)   1 mirrored rows used.
 * With augment == 0 and mirror_coef == 0 the mirrored rows add exact zeros: the gradients are tsidb_policy_learn's bit for bit.
 * With augment != 0, mirror_coef == 0 and M a multiple of 16 they are, bit for bit, tsidb_policy_learn's on a storage of twice
 * the rows whose second half holds the mirrored rows, with index2 = (index, index + rows).
 * workspace: at least tsidb_policy_learn_sym_workspace's bytes.  With Mp = M rounded up to a multiple of 16 every per-row array
 * has 2 Mp rows, the originals in [0, Mp), the mirrors in [Mp, 2 Mp): the first 2 Mp * NA floats are mu, the next 2 Mp are v
 * (with a critic; its mirrored half is 0 without augment).  The weight gradient runs over the 2 Mp rows in segments of
 * TSIDB_POL_LEARN_SEG_ROWS in that order.
 * Rejects: what tsidb_policy_learn rejects; a NULL actor or action table, a NULL critic table with a critic, a NULL sym->stats;
 * a negative or non-finite mirror_coef; M above 2^29.  sym NULL is tsidb_policy_learn (tsidb_policy_learn_workspace's bytes). */
enum { TSIDB_POL_SYM_NSTATS = 2 };
typedef struct tsidb_policy_symmetry {
  const int32_t *actor_perm;
  const float *actor_sign;
  const int32_t *critic_perm;
  const float *critic_sign;
  const int32_t *action_perm;
  const float *action_sign;
  int augment;
  float mirror_coef;              /* >= 0 */
  float *stats;                   /* [TSIDB_POL_SYM_NSTATS] */
} tsidb_policy_symmetry;

int tsidb_policy_learn_sym_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes);

int tsidb_policy_learn_sym(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                           const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                           const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                           const tsidb_policy_learn_cfg *cfg, const tsidb_policy_symmetry *sym, float *workspace,
                           size_t workspace_bytes, float *stats, void *stream);

/* ---- the step's side of a PPO iteration: what rsl_rl runs per minibatch behind the loss - its adaptive step size from the
 * exact Gaussian KL (schedule = "adaptive"), torch's clip_grad_norm_ over all parameters, and torch.optim.Adam's default
 * single-tensor step - as three plain asynchronous launches on the given stream: no atomics, no counters, no allocation, no
 * host synchronisation, capturable in a graph; every sum has one fixed order, two calls from the same state write the same bits.
 *
 * The parameter set, P elements in this order: the actor's layers (weight, then bias where the network has one), the critic's
 * layers, log_std [NA].  Weights and biases are the pointers of tsidb_policy_net and ARE WRITTEN IN PLACE ("read in place"
 * turned round: the next tsidb_policy_actor / tsidb_policy_learn launch computes with the step); the gradients - actor_grads,
 * critic_grads, log_std_grad, as tsidb_policy_learn wrote them - are READ ONLY, the clip factor is applied inside the step.
 * State, device memory the caller owns (tsidb_policy_opt_state):
 *   moments [2, P] float32   exp_avg then exp_avg_sq, the pieces in the order above        initial 0
 *   lr [1] float32, step [1] int64 (initial 0), log_std_old [NA] float32 (the rollout's log_std; the schedule alone reads it),
 *   stats [TSIDB_POL_OPT_NSTATS] float32, written by every call.
 *
 * One call, float32 unless said otherwise:
 * NORM.  norm = sqrt(sum g^2) over every gradient element, squares and sums in float64.  Each piece is cut into chunks of
 * TSIDB_POL_OPT_CHUNK elements (the last one ragged; elements beyond it count as 0).  A chunk's sum: element 4 t + i belongs to
 * slot t of TSIDB_POL_OPT_LANES; slot sum = ((g_0^2 + g_1^2) + g_2^2) + g_3^2; then the slots are halved,
 * slot[t] += slot[t + s] for t < s, s = LANES / 2, LANES / 4 .. 1.  The chunk sums are added in chunk order (piece after piece).
 *   coef = min(1, max_norm / (norm + 1e-6)) in float64, cast once (a NaN stays a NaN); max_norm = 0: coef = 1, no clipping.
 * KL, only with desired_kl > 0, over the M rows of the learner's last minibatch (tsidb_policy_opt_kl): mu = the first floats of
 * the learner's workspace, mu[m * NA + a]; mu_old = mean[index[m] * NA + a] of the rollout's stored [rows, NA] means; s =
 * log_std, s_old = log_std_old; in float64 from those float32 values
 *   kl_m = sum_a ( s_a - s_old_a + (exp(2 s_old_a) + (mu_old - mu)^2) / (2 exp(2 s_a)) - 1/2 )   in rising a;   kl = (sum_m kl_m) / M
 * Rows are cut into segments of TSIDB_POL_LEARN_SEG_ROWS; slot t of a segment = kl of its row t + kl of its row t + LANES, the
 * slots halved as above, the segments added in order.  An index outside [0, rows) contributes nothing; the mean stays over M.
 * STEP SIZE, rsl_rl's rule, before the step that uses it; the comparisons on the float64 kl, lr in IEEE float32, read from and
 * written to device memory:
 *   kl > 2 desired_kl: lr = max(lr_min, lr / 1.5f);   else 0 < kl < desired_kl / 2: lr = min(lr_max, lr * 1.5f)
 * ADAM.  t = step + 1, g = coef * grad;  m += (g - m) (1 - b1);  v = b2 v + (1 - b2) g^2;  bc1 = 1 - b1^t, bc2 = 1 - b2^t (float64);
 *   p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))     with lr / bc1 and sqrt(bc2) formed in float64 and cast once;
 * then step = t.  No weight decay, no amsgrad.
 * SKIP.  skip_nonfinite set and norm (or, with the schedule, kl) not finite: parameters, moments, lr and step keep their bits,
 * stats[5] = 1.  Clear: the arithmetic runs as torch's would and poisons the parameters.
 * stats: 0 norm  1 coef  2 kl (0 without the schedule)  3 lr used  4 step after the call  5 skipped  6 rows that entered the KL
 *   7 the direction lr moved, -1 / 0 / +1 (0 where a bound held it)
 *
 * workspace: device memory of at least tsidb_policy_opt_workspace's bytes (a function of the networks and of M, the rows of the
 * KL; M = 0 without the schedule), rewritten by every call: nchunks + 2 nseg float64 partial sums (nchunks = the chunks of all
 * pieces, nseg = ceil(M / TSIDB_POL_LEARN_SEG_ROWS)), then norm and kl in float64 as they were formed, before stats' float32
 * cast; the rest is the library's.  kl may be NULL without the schedule.
 * Rejects (message via tsidb_last_error, nothing launched): a NULL actor, actor_grads, cfg, state, log_std, log_std_grad,
 * moments, lr, step, stats or workspace; critic_grads NULL with a critic; what tsidb_policy_learn rejects in a network; a NULL
 * weight gradient, a NULL bias gradient where the bias exists; b1 or b2 outside [0, 1); eps <= 0; max_norm < 0; desired_kl < 0;
 * lr_min <= 0 or lr_min > lr_max; the schedule without kl, mean, index, mu or log_std_old, or with M < 1 or rows < 1; a
 * workspace smaller than the query's. */
enum { TSIDB_POL_OPT_CHUNK = 1024, TSIDB_POL_OPT_LANES = 256, TSIDB_POL_OPT_NSTATS = 8 };
typedef struct tsidb_policy_opt_cfg {
  double b1;
  double b2;
  double eps;
  double max_norm;           /* 0 = no clipping */
  double desired_kl;         /* 0 = no schedule */
  float lr_min;
  float lr_max;
  int skip_nonfinite;
} tsidb_policy_opt_cfg;

typedef struct tsidb_policy_opt_state {
  float *moments;            /* [2, P] */
  float *lr;                 /* [1] */
  int64_t *step;             /* [1] */
  const float *log_std_old;  /* [NA] */
  float *stats;              /* [8] */
} tsidb_policy_opt_state;

typedef struct tsidb_policy_opt_kl {
  const float *mu;           /* the learner's workspace: [Mp, NA] first */
  const float *mean;         /* [rows, NA] the rollout's stored means */
  const int32_t *index;      /* [M] device */
  int rows;
  int M;
} tsidb_policy_opt_kl;

int tsidb_policy_opt_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes);

int tsidb_policy_opt_step(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                          const tsidb_policy_grads *actor_grads, const tsidb_policy_grads *critic_grads, float *log_std,
                          const float *log_std_grad, const tsidb_policy_opt_cfg *cfg, const tsidb_policy_opt_state *state,
                          const tsidb_policy_opt_kl *kl, void *workspace, size_t workspace_bytes, void *stream);

/* probe of formulation.computeProblemData's rigid-body terms (main.py:119): M [N,26,26],
 * hbias [N,26], Jcom [N,3,26], Jf [N,2,6,26] (LOCAL), oMf [N,2,12], com [N,3].  Test/debug use. */
int tsidb_rbd_terms(tsidb_handle h, const void *q, const void *v, void *M, void *hbias, void *Jcom, void *Jf,
                    void *oMf, void *com, void *stream);

/* dimensions of the robot this library was built for (one library per robot: libtsidb.so = the v1 robot of ctrl/conf.py:9-15,
 * libtsidb_v0.so = robot/v0): out9 = NJ, NQ, NV, NA, sim bodies, 1 if the sim stage is built, collision geoms, contact
 * dimension, 1 if joints are damped - the nine ints of the blob's model_dims section, which tsidb_create compares.  The
 * TSIDB_N* constants above are the v1 robot's. */
int tsidb_dims(int *out9);

/* bytes of LDS one env occupies in kernel `which` (0 tick, 1 sim) for `dtype` */
int tsidb_lds_bytes(int dtype, int which);

#ifdef __cplusplus
}
#endif
#endif
