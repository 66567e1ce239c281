"""ctypes binding of libtsidb.so (include/tsidb.h).  There is no CPU fallback: if the HIP library
is missing or a call fails, this raises."""
import ctypes as C
from pathlib import Path

_HERE = Path(__file__).parent
import os

# TSIDB_LIB_PATH selects a diagnostic build (tools/stamp_profile.py); the product default is in-tree
LIB_PATH = Path(os.environ.get("TSIDB_LIB_PATH", _HERE / "libtsidb.so"))

SYMBOLS = ["tsidb_dims", "tsidb_create", "tsidb_destroy", "tsidb_last_error", "tsidb_set_params", "tsidb_set_refs", "tsidb_reset",
           "tsidb_tick", "tsidb_sim", "tsidb_step", "tsidb_rbd_terms", "tsidb_lds_bytes", "tsidb_walk_update", "tsidb_set_env_params", "tsidb_set_cop_ref",
           "tsidb_reset_done", "tsidb_set_posture_bias", "tsidb_walk_plan", "tsidb_set_option", "tsidb_tick_walk", "tsidb_sim_batch", "tsidb_stream_create", "tsidb_stream_destroy", "tsidb_get_option",
           "tsidb_set_xfrc", "tsidb_set_sim_readouts", "tsidb_set_sensors", "tsidb_set_ctrl", "tsidb_sim_ctrl",
           "tsidb_policy_config", "tsidb_policy_act", "tsidb_policy_reward", "tsidb_policy_obs",
           "tsidb_policy_randomize", "tsidb_policy_perturb", "tsidb_policy_reset_noise",
           "tsidb_policy_teacher_config", "tsidb_policy_teacher", "tsidb_policy_teacher_obs",
           "tsidb_policy_terrain_config", "tsidb_policy_terrain_reset", "tsidb_policy_height_scan",
           "tsidb_policy_actor", "tsidb_policy_gae", "tsidb_policy_learn_workspace", "tsidb_policy_learn",
           "tsidb_policy_norm_workspace", "tsidb_policy_norm_update", "tsidb_policy_actor_norm",
           "tsidb_policy_opt_workspace", "tsidb_policy_opt_step",
           "tsidb_policy_teacher_mix", "tsidb_policy_learn_imit_workspace", "tsidb_policy_learn_imit",
           "tsidb_policy_episode_config", "tsidb_policy_episode_end", "tsidb_policy_episode_begin",
           "tsidb_policy_obs_history", "tsidb_policy_learn_sym_workspace", "tsidb_policy_learn_sym"]

# tsidb_set_option / tsidb_get_option numbers (include/tsidb.h TSIDB_OPT_*; 4 is retired) and tsidb_stream_create roles
OPT_SIM_WAVES, OPT_LDS_PAD, OPT_CU_SPLIT, OPT_QP_FAST_EQ = 1, 2, 3, 5
ROLE_TICK, ROLE_SIM = 0, 1
# tsidb_set_ctrl modes (include/tsidb.h TSIDB_CTRL_*) and the most sim steps one launch takes (TSIDB_MAX_SIM_BATCH)
CTRL_OFF, CTRL_POSITION, CTRL_MOTOR, CTRL_RESIDUAL = 0, 1, 2, 3
CTRL_MODES = {"position": CTRL_POSITION, "motor": CTRL_MOTOR, "residual": CTRL_RESIDUAL}
MAX_SIM_BATCH = 8
# the policy environment (include/tsidb.h TSIDB_POL_*): reward terms in the order of the terms row and of the weights, slots of
# the action ring, privileged columns behind the observation, and the layout of tsidb_policy_config's parameter vector
POL_TERMS = ("track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "action_rate",
             "joint_vel", "feet_air_time", "alive", "termination")
POL_NT, POL_HIST, POL_NPRIV = 12, 8, 4
POL_P_CLIP, POL_P_ALPHA, POL_P_SIGMA, POL_P_H_TARGET, POL_P_T_AIR, POL_P_DEADBAND, POL_P_MAX_EPISODE_STEPS, POL_P_DECIMATION, \
    POL_P_SEED, POL_P_CMD_LO, POL_P_CMD_HI, POL_P_WEIGHTS, POL_NPARAMS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 27

# tsidb_policy_randomize's parameter vector (include/tsidb.h TSIDB_POL_DR_*), in its order; the two base velocity amplitudes
# take three slots each (x, y, z)
POL_DR_FIELDS = ("seed", "env_offset", "reset_joint_pos", "reset_joint_vel", "reset_base_lin_vel", "reset_base_ang_vel", "reset_yaw",
                 "reset_xy", "reset_lift", "noise_ang_vel", "noise_gravity", "noise_joint_pos", "noise_joint_vel", "push_interval",
                 "push_duration", "push_force_lo", "push_force_hi", "command_interval", "command_zero_prob")
POL_DR_SEED, POL_DR_ENV_OFFSET, POL_DR_RESET_JOINT_POS, POL_DR_RESET_JOINT_VEL, POL_DR_RESET_BASE_LIN_VEL, POL_DR_RESET_BASE_ANG_VEL, \
    POL_DR_RESET_YAW, POL_DR_RESET_XY, POL_DR_RESET_LIFT, POL_DR_NOISE_ANG_VEL, POL_DR_NOISE_GRAVITY, POL_DR_NOISE_JOINT_POS, \
    POL_DR_NOISE_JOINT_VEL, POL_DR_PUSH_INTERVAL, POL_DR_PUSH_DURATION, POL_DR_PUSH_FORCE_LO, POL_DR_PUSH_FORCE_HI, \
    POL_DR_COMMAND_INTERVAL, POL_DR_COMMAND_ZERO_PROB, POL_DR_NPARAMS = 0, 1, 2, 3, 4, 7, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23

# tsidb_policy_terrain_config's parameter vector (include/tsidb.h TSIDB_POL_TER_*), in its order, and the most points of a
# height scan (TSIDB_POL_MAXSCAN)
POL_TER_NAMES = ("seed", "env_offset", "mass_lo", "mass_hi", "friction_lo", "friction_hi", "tilt_max", "step_height_lo", "step_height_hi",
                 "step_length_lo", "step_length_hi", "step_prob", "flat_cells", "num_levels", "scan_nx", "scan_ny", "scan_x0", "scan_x1",
                 "scan_y0", "scan_y1", "scan_clip_lo", "scan_clip_hi", "scan_noise")
POL_TER_SEED, POL_TER_ENV_OFFSET, POL_TER_MASS_LO, POL_TER_MASS_HI, POL_TER_FRICTION_LO, POL_TER_FRICTION_HI, POL_TER_TILT_MAX, \
    POL_TER_STEP_HEIGHT_LO, POL_TER_STEP_HEIGHT_HI, POL_TER_STEP_LENGTH_LO, POL_TER_STEP_LENGTH_HI, POL_TER_STEP_PROB, POL_TER_FLAT_CELLS, \
    POL_TER_NUM_LEVELS, POL_TER_SCAN_NX, POL_TER_SCAN_NY, POL_TER_SCAN_X0, POL_TER_SCAN_X1, POL_TER_SCAN_Y0, POL_TER_SCAN_Y1, \
    POL_TER_SCAN_CLIP_LO, POL_TER_SCAN_CLIP_HI, POL_TER_SCAN_NOISE, POL_TER_NPARAMS = range(24)
POL_MAXSCAN = 256
# PolicyTerrain's fields (policy_env.py): ranges are (lo, hi) pairs, the scan axes (first, last, points)
POL_TER_FIELDS = ("seed", "env_offset", "mass", "friction", "tilt_deg", "step_height", "step_length", "step_prob", "flat_cells", "num_levels",
                  "scan_x", "scan_y", "scan_clip", "scan_noise")

# TSID in the loop of the policy environment (include/tsidb.h TSIDB_POL_TEACH_*): the teacher terms in the order of the
# teacher_terms row and of the weights, and the layout of tsidb_policy_teacher_config's parameter vector
POL_TEACH_TERMS = ("track_com", "track_feet", "contact_match", "deviation")
POL_TEACH_NT = 4
POL_TEACH_SIGMA_COM, POL_TEACH_SIGMA_FOOT, POL_TEACH_WEIGHTS, POL_TEACH_NPARAMS = 0, 1, 2, 6


# the policy actor (include/tsidb.h tsidb_policy_net): the most layers, input blocks and columns of a layer or of the input row,
# the hidden activations, tsidb_policy_actor's flag, and the two streams of the action noise
POL_NET_MAXLAYERS, POL_NET_MAXBLOCKS, POL_NET_MAXWIDTH = 4, 4, 512
POL_ACTIVATIONS = ("elu", "tanh", "relu")
POL_ACTOR_SAMPLE = 1
POL_ACTOR_STREAMS = (21, 22)
# the policy learner (include/tsidb.h tsidb_policy_learn): the rows of a segment of the weight gradient's sums, and the stats
POL_LEARN_SEG_ROWS = 512
POL_LEARN_STATS = ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "loss", "rows", "bad_indices")
# imitation of the teacher (include/tsidb.h tsidb_policy_teacher_mix, tsidb_policy_learn_imit): the stream of the per-episode
# teacher / student draw, the losses in the order of TSIDB_POL_IMIT_*, and the imitation stats
POL_TEACHER_MIX_STREAM = 23
POL_IMIT_LOSSES = ("mse", "huber")
POL_IMIT_STATS = ("imitation_loss", "weight_sum", "weighted_rows", "skipped_rows")
# the mirror symmetry (include/tsidb.h tsidb_policy_learn_sym): its stats
POL_SYM_STATS = ("mirror_loss", "mirrored_rows")
# episode statistics and the terrain curriculum (include/tsidb.h TSIDB_POL_EP_*, TSIDB_POL_EPP_*): the columns of an episode's
# record, tsidb_policy_episode_config's parameter vector, PolicyCurriculum's fields and the stream of a graduate's level
POL_EP_COUNT, POL_EP_TIMEOUT, POL_EP_LENGTH, POL_EP_RETURN, POL_EP_DISPLACEMENT, POL_EP_LEVEL, POL_EP_TERMS, POL_EP_TEACH, POL_EP_NREC = \
    0, 1, 2, 3, 4, 5, 6, 18, 22
POL_EPP_CURRICULUM, POL_EPP_UP_DISTANCE, POL_EPP_DOWN_FRACTION, POL_EPP_RANDOM_TOP, POL_EPP_NPARAMS = range(5)
POL_CURRICULUM_FIELDS = ("up_distance", "down_fraction", "random_top")
POL_CURRICULUM_STREAM = 24
# the observation history (include/tsidb.h tsidb_policy_obs_history, TSIDB_POL_OBSH_*): the most sources of a frame, frames and
# columns of a history row, the tensors of a PolicyEnv a source may name, and PolicyObsHistory's fields
POL_OBSH_MAXSRC, POL_OBSH_MAXFRAMES, POL_OBSH_MAXCOLS = 4, 32, 4096
POL_OBSH_SOURCES = ("obs", "priv", "command", "height_scan", "teacher_obs")
POL_OBSH_FIELDS = ("frames", "sources")
# the policy normaliser (include/tsidb.h tsidb_policy_norm_update): the rows of a segment of the batch statistics
POL_NORM_SEG_ROWS = 256
# the policy optimiser (include/tsidb.h tsidb_policy_opt_step): the elements of a chunk of the gradient norm's sums, the slots
# of a chunk's (and of a KL segment's) sum, and the stats
POL_OPT_CHUNK, POL_OPT_LANES = 1024, 256
POL_OPT_STATS = ("grad_norm", "clip_coef", "kl", "lr", "step", "skipped", "kl_rows", "lr_direction")


def pol_teach_nobs(na):
    """columns of the teacher observation for a robot with na actuators (TSIDB_POL_TEACH_NOBS is the v1 robot's)"""
    return 14 + na


def pol_nobs(na):
    """observation columns of the policy environment for a robot with na actuators (TSIDB_POL_NOBS is the v1 robot's)"""
    return 11 + 3 * na

_libs = {}


class TsidbError(RuntimeError):
    pass


class WalkArgs(C.Structure):
    """tsidb_walk_args (include/tsidb.h): tsidb_walk_update's arguments as one block"""
    _fields_ = [("coef", C.c_void_p), ("side", C.c_void_p), ("nsteps", C.c_void_p), ("rest", C.c_void_p), ("com", C.c_void_p),
                ("K", C.c_int), ("t", C.c_double), ("step_duration", C.c_double), ("t_start", C.c_double), ("omega", C.c_double),
                ("com_z0", C.c_double), ("com_drop", C.c_double), ("frames", C.c_void_p), ("t_offset", C.c_void_p),
                ("ncon", C.c_void_p), ("con_pairs", C.c_void_p), ("td_latch", C.c_void_p), ("td_fraction", C.c_double),
                ("t_device", C.c_void_p)]


class PolicyBufs(C.Structure):
    """tsidb_policy_bufs (include/tsidb.h): the per-env state of the policy environment"""
    _fields_ = [("act_hist", C.c_void_p), ("last_action", C.c_void_p), ("prev_action", C.c_void_p), ("command", C.c_void_p),
                ("air_time", C.c_void_p), ("ep_len", C.c_void_p), ("episode", C.c_void_p), ("delay", C.c_void_p),
                ("terms", C.c_void_p), ("timeout", C.c_void_p), ("obs", C.c_void_p), ("obs_ld", C.c_int)]


class PolicyEpisode(C.Structure):
    """tsidb_policy_episode (include/tsidb.h): the per-env episode state of the statistics and the curriculum"""
    _fields_ = [("run", C.c_void_p), ("start_xy", C.c_void_p), ("last", C.c_void_p), ("sum", C.c_void_p), ("level", C.c_void_p),
                ("teacher_terms", C.c_void_p)]


class PolicyObsHistory(C.Structure):
    """tsidb_policy_obs_history (include/tsidb.h): the history rows and the column blocks a frame is made of"""
    _fields_ = [("history", C.c_void_p), ("frames", C.c_int), ("n_src", C.c_int), ("src", C.c_void_p * 4), ("src_ld", C.c_int * 4),
                ("src_cols", C.c_int * 4)]


class PolicyNet(C.Structure):
    """tsidb_policy_net (include/tsidb.h): a dense network, its parameters in place, and the column blocks of its input row"""
    _fields_ = [("n_layers", C.c_int), ("width", C.c_int * 4), ("activation", C.c_int), ("weight", C.c_void_p * 4),
                ("bias", C.c_void_p * 4), ("n_blocks", C.c_int), ("block", C.c_void_p * 4), ("block_ld", C.c_int * 4),
                ("block_cols", C.c_int * 4)]


class PolicyActorOut(C.Structure):
    """tsidb_policy_actor_out (include/tsidb.h): what tsidb_policy_actor writes, every pointer optional"""
    _fields_ = [("action", C.c_void_p), ("action32", C.c_void_p), ("mean", C.c_void_p), ("logp", C.c_void_p), ("value", C.c_void_p),
                ("actor_input", C.c_void_p), ("critic_input", C.c_void_p)]


class PolicyNorm(C.Structure):
    """tsidb_policy_norm (include/tsidb.h): one network's normaliser state and settings"""
    _fields_ = [("affine", C.c_void_p), ("clip", C.c_float), ("stats", C.c_void_p), ("count", C.c_void_p), ("eps", C.c_double),
                ("until", C.c_int64)]


class PolicyLearnBatch(C.Structure):
    """tsidb_policy_learn_batch (include/tsidb.h): the stored arrays of a rollout and the minibatch's rows"""
    _fields_ = [("actor_input", C.c_void_p), ("critic_input", C.c_void_p), ("action", C.c_void_p), ("logp", C.c_void_p),
                ("value", C.c_void_p), ("advantage", C.c_void_p), ("returns", C.c_void_p), ("index", C.c_void_p),
                ("rows", C.c_int), ("M", C.c_int), ("adv_stats", C.c_void_p)]


class PolicyGrads(C.Structure):
    """tsidb_policy_grads (include/tsidb.h): where the gradient of each layer's weight and bias goes"""
    _fields_ = [("weight", C.c_void_p * 4), ("bias", C.c_void_p * 4)]


class PolicyLearnCfg(C.Structure):
    """tsidb_policy_learn_cfg (include/tsidb.h)"""
    _fields_ = [("clip", C.c_float), ("value_coef", C.c_float), ("entropy_coef", C.c_float), ("value_clip", C.c_int)]


class PolicySymmetryTables(C.Structure):
    """tsidb_policy_symmetry (include/tsidb.h): the signed permutations of tsidb_policy_learn_sym and its two switches"""
    _fields_ = [("actor_perm", C.c_void_p), ("actor_sign", C.c_void_p), ("critic_perm", C.c_void_p), ("critic_sign", C.c_void_p),
                ("action_perm", C.c_void_p), ("action_sign", C.c_void_p), ("augment", C.c_int), ("mirror_coef", C.c_float),
                ("stats", C.c_void_p)]


class PolicyImit(C.Structure):
    """tsidb_policy_imit (include/tsidb.h): the imitation term of tsidb_policy_learn_imit"""
    _fields_ = [("target", C.c_void_p), ("weight", C.c_void_p), ("skip_surrogate", C.c_void_p), ("imitation_coef", C.c_float),
                ("surrogate_coef", C.c_float), ("loss", C.c_int), ("stats", C.c_void_p)]


class PolicyOptCfg(C.Structure):
    """tsidb_policy_opt_cfg (include/tsidb.h)"""
    _fields_ = [("b1", C.c_double), ("b2", C.c_double), ("eps", C.c_double), ("max_norm", C.c_double), ("desired_kl", C.c_double),
                ("lr_min", C.c_float), ("lr_max", C.c_float), ("skip_nonfinite", C.c_int)]


class PolicyOptState(C.Structure):
    """tsidb_policy_opt_state (include/tsidb.h): the optimiser's device memory"""
    _fields_ = [("moments", C.c_void_p), ("lr", C.c_void_p), ("step", C.c_void_p), ("log_std_old", C.c_void_p), ("stats", C.c_void_p)]


class PolicyOptKl(C.Structure):
    """tsidb_policy_opt_kl (include/tsidb.h): the learner's last minibatch, as the KL of the adaptive step size reads it"""
    _fields_ = [("mu", C.c_void_p), ("mean", C.c_void_p), ("index", C.c_void_p), ("rows", C.c_int), ("M", C.c_int)]


def dims9(L):
    """the nine ints a library was built for, in the order of the blob's model_dims section:
    NJ, NQ, NV, NA, sim bodies, has_sim, collision geoms, contact dimension, damped joints"""
    out = (C.c_int * 9)()
    L.tsidb_dims(out)
    return tuple(out)


def dims(L):
    """(NJ, NQ, NV, NA, sim bodies, has_sim) of the robot a loaded library was built for"""
    return dims9(L)[:6]


def load_for(model_dims):
    """The library built for a blob's robot (its model_dims section): one libtsidb*.so per robot sits next to this file
    (libtsidb.so = the v1 robot, libtsidb_v0.so = robot/v0).  TSIDB_LIB_PATH (diagnostic builds) is tried first."""
    want = tuple(int(x) for x in model_dims)[:9]   # all nine: two builds may differ in geoms / condim / damping only
    cands = [LIB_PATH] + sorted(p for p in _HERE.glob("libtsidb*.so") if p != LIB_PATH)
    for p in cands:
        if p.exists():
            L = load(p)
            if dims9(L)[:len(want)] == want:
                return L
    raise TsidbError(f"no libtsidb*.so in {_HERE} is built for a robot with dimensions {want}: compile the blob's topology "
                     "header into a library (python -c 'import __graft_entry__ as g; g.build()')")


def load(path=None):
    """Load a libtsidb*.so once (default: libtsidb.so, the v1 robot); raise loudly when it has not been built."""
    path = Path(path) if path is not None else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not path.exists():
        raise TsidbError(f"{path} is missing: build the HIP extension first "
                         "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU path")
    # torch first: its bundled HIP runtime must be the one this process initialises - the library is handed torch's device
    # pointers and streams, and loaded before torch it would bind /opt/rocm's libamdhip64 instead (a second runtime in one
    # process: hipGetDeviceCount then finds no device)
    import torch  # noqa: F401
    L = C.CDLL(str(path))
    vp, i32p = C.c_void_p, C.c_void_p
    L.tsidb_create.argtypes = [vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.tsidb_destroy.argtypes = [vp]
    L.tsidb_last_error.argtypes = [vp]
    L.tsidb_last_error.restype = C.c_char_p
    L.tsidb_set_params.argtypes = [vp, vp, C.c_int]
    L.tsidb_set_refs.argtypes = [vp] * 7
    L.tsidb_reset.argtypes = [vp, i32p, C.c_int, vp, vp, vp, vp, vp, vp]
    L.tsidb_tick.argtypes = [vp] * 8 + [C.c_int] + [vp] * 3
    L.tsidb_sim.argtypes = [vp] * 11
    L.tsidb_step.argtypes = [vp] * 11 + [C.c_int] + [vp] * 4 + [C.c_int, vp]
    L.tsidb_rbd_terms.argtypes = [vp] * 10
    L.tsidb_lds_bytes.argtypes = [C.c_int, C.c_int]
    L.tsidb_set_env_params.argtypes = [vp, vp, vp]
    L.tsidb_set_xfrc.argtypes = [vp, vp]
    L.tsidb_set_sim_readouts.argtypes = [vp] * 6
    L.tsidb_set_ctrl.argtypes = [vp, vp, C.c_int]
    L.tsidb_sim_ctrl.argtypes = [vp, C.c_int] + [vp] * 8
    L.tsidb_policy_config.argtypes = [vp, vp, C.c_int, vp, vp, C.c_uint32]
    L.tsidb_policy_act.argtypes = [vp, vp, vp, vp]
    L.tsidb_policy_reward.argtypes = [vp, vp, vp, vp, i32p, i32p, i32p, vp, vp, C.c_int, vp]
    L.tsidb_policy_obs.argtypes = [vp, vp, vp, C.c_int, vp, vp, i32p, i32p, vp]
    L.tsidb_policy_randomize.argtypes = [vp, vp, C.c_int]
    L.tsidb_policy_perturb.argtypes = [vp, vp, vp]
    L.tsidb_policy_reset_noise.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.tsidb_policy_teacher_config.argtypes = [vp, vp, C.c_int]
    L.tsidb_policy_teacher.argtypes = [vp, vp, vp, C.c_int, vp, vp, i32p, i32p, i32p, vp, vp, vp]
    L.tsidb_policy_teacher_obs.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.tsidb_policy_terrain_config.argtypes = [vp, vp, C.c_int]
    L.tsidb_policy_terrain_reset.argtypes = [vp, vp, vp, C.c_int, vp, i32p, vp]
    L.tsidb_policy_height_scan.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    L.tsidb_policy_actor.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp]
    L.tsidb_policy_gae.argtypes = [vp, C.c_int, vp, vp, i32p, vp, C.c_float, C.c_float, vp, vp, vp]
    L.tsidb_policy_learn_workspace.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
    L.tsidb_policy_learn.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp]
    L.tsidb_policy_teacher_mix.argtypes = [vp, vp, vp, vp, vp, vp, i32p, vp, C.c_uint64, C.c_uint64, vp]
    L.tsidb_policy_episode_config.argtypes = [vp, vp, C.c_int]
    L.tsidb_policy_episode_end.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.tsidb_policy_episode_begin.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
    L.tsidb_policy_obs_history.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.tsidb_policy_learn_imit_workspace.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
    L.tsidb_policy_learn_imit.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp]
    L.tsidb_policy_learn_sym_workspace.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
    L.tsidb_policy_learn_sym.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp]
    L.tsidb_policy_norm_workspace.argtypes = [vp, vp, vp, C.POINTER(C.c_size_t)]
    L.tsidb_policy_norm_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.tsidb_policy_actor_norm.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp]
    L.tsidb_policy_opt_workspace.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
    L.tsidb_policy_opt_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.tsidb_set_sensors.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.tsidb_set_cop_ref.argtypes = [vp, vp]
    L.tsidb_walk_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int] + [C.c_double] * 6 + [vp, vp, vp, vp, vp, C.c_double, vp, vp]
    L.tsidb_dims.argtypes = [C.POINTER(C.c_int)]
    L.tsidb_reset_done.argtypes = [vp, vp, C.c_int] + [vp] * 7
    L.tsidb_set_posture_bias.argtypes = [vp, vp]
    L.tsidb_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.tsidb_sim_batch.argtypes = [vp, C.c_int] + [vp] * 11
    L.tsidb_tick_walk.argtypes = [vp, vp] + [vp] * 7 + [C.c_int] + [vp] * 5
    L.tsidb_walk_plan.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int] + [vp] * 9 + \
                                 [C.c_double, vp, vp]
    for s in SYMBOLS:
        if s != "tsidb_last_error":
            getattr(L, s).restype = C.c_int
    _libs[path] = L
    return L


def check(L, handle, rc, what):
    if rc != 0:
        msg = L.tsidb_last_error(handle)
        raise TsidbError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
