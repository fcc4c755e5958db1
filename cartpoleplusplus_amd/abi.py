"""ctypes mirror of include/cartpole_amd.h (structs, constants, layouts).

Pure data definitions: no library is loaded here.  `native.py` binds the HIP
library's entry points with these types.
"""
import ctypes as C

CP_ABI_VERSION = 8

CP_BODY_GROUND, CP_BODY_CART, CP_BODY_POLE, CP_BODY_CART2, CP_BODY_POLE2 = range(5)
CP_NUM_BODIES = 5
CP_NUM_DYN = 4
CP_NUM_PAIRS = 10
CP_NUM_ISLANDS = 2
CP_ISLAND_PAIRS = 5
CP_BODY_FIELDS = 13
CP_ISLAND_POINTS = 10
CP_ISLAND_FRICTION = 5
# global pair index of island p's local pair j (own 3, then its 2 cross pairs)
ISLAND_PAIR = ((0, 1, 4, 5, 6), (2, 3, 9, 7, 8))
CP_NUM_DISCRETE = 5


def CP_SF_BODY(dyn, c):
    return dyn * CP_BODY_FIELDS + c


def CP_SF_PENDING(cart, c):
    return CP_NUM_DYN * CP_BODY_FIELDS + cart * 3 + c


CP_SF_STEPS = CP_NUM_DYN * CP_BODY_FIELDS + 6
CP_SF_EPISODE = CP_SF_STEPS + 1
CP_SF_DONE = CP_SF_STEPS + 2


def CP_SF_WS_ID(isl, j):
    return CP_SF_STEPS + 3 + isl * CP_ISLAND_PAIRS + j


def CP_SF_WS_LAM(isl, j, k):
    return CP_SF_STEPS + 3 + CP_NUM_PAIRS + (isl * CP_ISLAND_PAIRS + j) * 4 + k


def CP_SF_SLEEP_ACT(dyn):
    return CP_SF_STEPS + 3 + CP_NUM_PAIRS * 5 + dyn


def CP_SF_SLEEP_TIMER(dyn):
    return CP_SF_STEPS + 3 + CP_NUM_PAIRS * 5 + CP_NUM_DYN + dyn


CP_STATE_FIELDS = CP_SF_STEPS + 3 + CP_NUM_PAIRS * 5 + 2 * CP_NUM_DYN
CP_ACT_ACTIVE, CP_ACT_SLEEPING, CP_ACT_WANTS, CP_ACT_AWAKE = 1, 2, 3, 16

CP_AUTORESET_OFF, CP_AUTORESET_SAME_STEP, CP_AUTORESET_NEXT_STEP = 0, 1, 2

CP_BUMP_PHILOX = 0
CP_BUMP_HOST = 1
CP_ACTION_CONTINUOUS = 0
CP_ACTION_DISCRETE = 1

# Discrete action table: order "no push, left, right, up, down"
# (bullet_cartpole.py:84,89); entry = unit (fx, fy) scaled by action_force.
DISCRETE_TABLE = ((0.0, 0.0), (-1.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.0, -1.0))

_F3 = C.c_float * 3


class cp_physics(C.Structure):
    _fields_ = [
        ("dt", C.c_float),
        ("inv_dt", C.c_float),
        ("gravity", _F3),
        ("lin_damping", C.c_float),
        ("ang_damping", C.c_float),
        ("erp", C.c_float),
        ("contact_margin", C.c_float),
        ("residual_threshold", C.c_float),
        ("solver_iterations", C.c_int32),
        ("edge_bias", C.c_float),
        ("max_angular_step", C.c_float),
        ("warmstart", C.c_float),
        ("half_extents", _F3 * CP_NUM_BODIES),
        ("inv_mass", C.c_float * CP_NUM_BODIES),
        ("inertia", _F3 * CP_NUM_BODIES),
        ("inv_inertia", _F3 * CP_NUM_BODIES),
        ("friction", C.c_float * CP_NUM_BODIES),
        ("spawn_pos", _F3 * CP_NUM_BODIES),
        ("model_flags", C.c_int32),
        ("max_coord_velocity", C.c_float),
        ("sleep_epsilon", C.c_float),
        ("sleep_timeout", C.c_float),
    ]


# cp_physics.model_flags: alternatives to the default contact model (oracle-only unless in
# CP_MODEL_GPU_FLAGS; DESIGN.md §3 sensitivity study)
CP_MODEL_SPLIT_ISLANDS = 0x1
CP_MODEL_VEL_FRICTION = 0x2
CP_MODEL_PERSISTENT = 0x4
CP_MODEL_SLEEPING = 0x8
CP_MODEL_GPU_FLAGS = 0xC

# kernel shapes (cp_set_kernel_shape)
CP_SHAPE_AUTO = -1
CP_SHAPE_THROUGHPUT = 0
CP_SHAPE_LATENCY = 1
CP_SHAPE_WIDE = 2
CP_SHAPE_WIDE8 = 3
CP_SHAPE_WIDE64 = 4
CP_SHAPE_LIST = 5   # reset lists: the layout picked on the device by the list's length (include/cartpole_amd.h)
SHAPES = {"auto": CP_SHAPE_AUTO, "throughput": CP_SHAPE_THROUGHPUT, "latency": CP_SHAPE_LATENCY, "wide": CP_SHAPE_WIDE,
          "wide8": CP_SHAPE_WIDE8, "wide64": CP_SHAPE_WIDE64, "list": CP_SHAPE_LIST}


class cp_config(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32),
        ("action_repeats", C.c_int32),
        ("steps_per_repeat", C.c_int32),
        ("max_episode_len", C.c_int32),
        ("action_force", C.c_float),
        ("initial_force", C.c_float),
        ("random_theta", C.c_int32),
        ("initial_force_steps", C.c_int32),
        ("settle_steps", C.c_int32),
        ("done_on_bounds", C.c_int32),
        ("pos_threshold", C.c_float),
        ("angle_threshold", C.c_float),
        ("tan_angle_threshold", C.c_float),
        ("sin_angle_threshold", C.c_float),
        ("autoreset", C.c_int32),
        ("bump_mode", C.c_int32),
        ("seed", C.c_uint64),
        ("env_id_offset", C.c_int64),
        ("phys", cp_physics),
        ("precision", C.c_int32),
        ("reset_flags", C.c_int32),
    ]


CP_RESET_CLEAR_NONFINITE_FORCE = 0x1


CP_PRECISION_F32 = 0
CP_PRECISION_F64 = 1


class cp_raster_config(C.Structure):
    """include/cartpole_amd.h: cp_raster_config (raster obs, bullet_cartpole.py:277-306)."""
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("num_cameras", C.c_int32),
        ("eye", _F3 * 2),
        ("target", _F3),
        ("up", _F3),
        ("tan_half_fov", C.c_float),
        ("far_plane", C.c_float),
        ("light", _F3),
        ("ambient", C.c_float),
        ("diffuse", C.c_float),
        ("background", _F3),
        ("color", _F3 * CP_NUM_BODIES),
    ]


# ---- in-kernel MLP policy (include/cartpole_amd.h: cp_policy)
CP_POLICY_MAX_LAYERS = 4
CP_POLICY_MAX_WIDTH = 128
CP_HEAD_TANH, CP_HEAD_CLIP, CP_HEAD_ARGMAX, CP_HEAD_SAMPLE = range(4)
HEADS = {"tanh": CP_HEAD_TANH, "clip": CP_HEAD_CLIP, "argmax": CP_HEAD_ARGMAX, "sample": CP_HEAD_SAMPLE}


class cp_policy(C.Structure):
    _fields_ = [
        ("num_layers", C.c_int32),
        ("width", C.c_int32 * (CP_POLICY_MAX_LAYERS + 1)),
        ("head", C.c_int32),
        ("epsilon", C.c_float),
        ("seed", C.c_uint64),
        ("weights", C.c_void_p),
        ("population", C.c_int32),
        ("group", C.c_int32),
    ]


# ---- in-kernel exploration noise of the continuous heads (include/cartpole_amd.h: cp_policy_noise)
CP_NOISE_OFF, CP_NOISE_GAUSSIAN, CP_NOISE_OU = range(3)
CP_NOISE_RESET_ON_EPISODE = 0x1
CP_NOISE_CLIP_SYMMETRIC = 0x2
NOISE_KINDS = {"off": CP_NOISE_OFF, "gaussian": CP_NOISE_GAUSSIAN, "ou": CP_NOISE_OU}


class cp_policy_noise(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("flags", C.c_int32),
        ("theta", C.c_float),
        ("sigma", C.c_float),
        ("max_magnitude", C.c_float),
        ("seed", C.c_uint64),
    ]


# ---- seeded ES perturbations of the policy's centre (include/cartpole_amd.h: cp_policy_es)
CP_ES_OFF, CP_ES_BYTES4 = range(2)
CP_ES_ANTITHETIC = 0x1


class cp_policy_es(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("flags", C.c_int32),
        ("sigma", C.c_float),
        ("generation", C.c_uint32),
        ("seed", C.c_uint64),
        ("population", C.c_int32),
        ("group", C.c_int32),
    ]


def pixels_shape(B, H, W, C_, R):
    """Raster obs per env (H, W, 3, C, R), bullet_cartpole.py:299-306 (camera before repeat)."""
    return (B, H, W, 3, C_, R)


def obs_shape(B, R):
    return (B, R, 2, 7)


def readback_shape(B, R, S):
    return (B, 2, R, S, 4, 3)


# ---- replay memory (include/cartpole_amd.h: cp_replay)
CP_RM_INSERT, CP_RM_FULL, CP_RM_HEAD, CP_RM_TAIL, CP_RM_ERROR, CP_RM_ADDS, CP_RM_EVICTED_S2 = range(7)
CP_RM_CTRL = 8
CP_STATES_F32 = 0
CP_STATES_F16 = 1


class cp_replay(C.Structure):
    _fields_ = [
        ("buffer_size", C.c_int32),
        ("state_buffer_size", C.c_int32),
        ("state_dim", C.c_int32),
        ("action_dim", C.c_int32),
        ("state", C.c_void_p),
        ("state_1_idx", C.c_void_p),
        ("action", C.c_void_p),
        ("reward", C.c_void_p),
        ("terminal_mask", C.c_void_p),
        ("state_2_idx", C.c_void_p),
        ("free_slots", C.c_void_p),
        ("ctrl", C.c_void_p),
        ("plan", C.c_void_p),
        ("scan", C.c_void_p),
    ]


class cp_replay_batch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("idx", "state_1", "action", "reward", "terminal_mask", "state_2",
                                          "state_1_idx", "state_2_idx")]


# ---- returns and advantages of a rollout window (include/cartpole_amd.h: cp_returns)
CP_RET_EPISODE_TOTAL, CP_RET_DISCOUNTED, CP_RET_GAE = range(3)
CP_RET_BOUNDARY_SAME_STEP, CP_RET_BOUNDARY_STICKY, CP_RET_BOUNDARY_NEXT_STEP = range(3)
CP_RET_MASK_OPEN = 0x1
CP_RET_STANDARDISE = 0x2
RET_KINDS = {"episode_total": CP_RET_EPISODE_TOTAL, "discounted": CP_RET_DISCOUNTED, "gae": CP_RET_GAE}
RET_BOUNDARIES = {"same_step": CP_RET_BOUNDARY_SAME_STEP, "sticky": CP_RET_BOUNDARY_STICKY,
                  "next_step": CP_RET_BOUNDARY_NEXT_STEP}


class cp_returns(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("boundary", C.c_int32),
        ("flags", C.c_uint32),
        ("gamma", C.c_float),
        ("lam", C.c_float),          # `lambda` in the header
        ("steps", C.c_int32),
        ("num_envs", C.c_int32),
        ("env_id_offset", C.c_int64),
        ("population", C.c_int32),
        ("group", C.c_int32),
    ]


def state_ints(values):
    """Integer state fields (steps, episode, done, warm-start ids) from a state array:
    float32 holds the int32 bits; a float64 state (fp64 build) holds them in the first 4
    bytes (the low word on this little-endian ABI) of each 8-byte field."""
    import numpy as np
    a = np.ascontiguousarray(values)
    if a.dtype == np.float64:
        return a.view(np.int32)[..., 0::2]
    return a.view(np.int32)
