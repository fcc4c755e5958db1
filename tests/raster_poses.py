"""Poses off the reference view for the raster tests (plain module, no fixtures): bodies behind the eye, across
the eye plane, around the eye, on screen and partly off screen, and the camera / scene configurations
they are rendered with.

The render kernels cull with a conservative screen rectangle per box (cp_raster.h box_rect: all corners
behind the eye -> no test, a corner at or behind the eye plane -> no culling, otherwise the clamped pixel
bounds); the poses of the first steps after a reset only ever reach its last branch.  classify() names the
branch a box takes (in float64, from the corner depths and screen coordinates), so that the tests can
state as a precondition that every branch is reached.
"""
import math

import numpy as np

from cartpoleplusplus_amd import abi, native

ALL_BEHIND, STRADDLING, EYE_INSIDE, ON_SCREEN, PARTLY_OFF = range(5)
CLASS_NAMES = ["all behind", "straddling the eye plane", "eye inside", "fully on screen", "partly off screen"]
B = 48
SCENES = ["default", "second", "cart", "squat"]


def raster_config(scene, width, height, num_cameras):
    """cp_raster_config of a scene: the reference cameras, or ("second") other eyes, target, field of view,
    light, shading weights, background and body colours."""
    rc = native.default_raster_config(width=width, height=height, num_cameras=num_cameras)
    if scene == "second":
        for c, eye in enumerate(((0.3, 0.2, 0.12), (-0.4, 0.5, 1.5))):
            for k in range(3):
                rc.eye[c][k] = eye[k]
        for k, v in enumerate((0.0, 0.0, 0.1)):
            rc.target[k] = v
        rc.tan_half_fov = math.tan(math.radians(35.0))
        light = np.array([-0.5, 0.2, 0.7])
        for k, v in enumerate(light / np.linalg.norm(light)):
            rc.light[k] = v
        rc.ambient, rc.diffuse = 0.35, 0.65
        for k, v in enumerate((0.1, 0.2, 0.45)):
            rc.background[k] = v
        colors = ((0.8, 0.8, 0.7), (0.1, 0.3, 0.9), (1.0, 0.6, 0.0), (0.5, 0.0, 0.5), (0.0, 0.9, 0.8))
        for b in range(abi.CP_NUM_BODIES):
            for k in range(3):
                rc.color[b][k] = colors[b][k]
    return rc


def place(state, rc):
    """Write the test poses into a reset state SoA (float32, in place), velocities zero.  default_rng(0); per env
    four bodies with unit quaternions from normalised normals.  Envs e % 4 == 0: the cart centred within
    +-0.02 of camera 0's eye (the eye is inside a box); e % 4 == 1: every body within 0.25 m of the camera
    target (on screen); the rest uniform in [-0.6, 1.5] x [-0.3, 1.5] x [0, 1.2]."""
    n = state.shape[1]
    rng = np.random.default_rng(0)
    pos = rng.uniform([-0.6, -0.3, 0.0], [1.5, 1.5, 1.2], (n, 4, 3))
    q = rng.normal(size=(n, 4, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    near_eye = rng.uniform(-0.02, 0.02, (n, 3))
    near_target = rng.uniform(-1.0, 1.0, (n, 4, 3)) * (0.25 / math.sqrt(3.0))
    eye0 = np.array([rc.eye[0][k] for k in range(3)], np.float64)
    target = np.array([rc.target[k] for k in range(3)], np.float64)
    e = np.arange(n)
    pos[e % 4 == 0, 0] = (eye0 + near_eye)[e % 4 == 0]
    pos[e % 4 == 1] = (target + near_target)[e % 4 == 1]
    for d in range(4):
        for k in range(3):
            state[abi.CP_SF_BODY(d, k)] = pos[:, d, k].astype(np.float32)
        for k in range(4):
            state[abi.CP_SF_BODY(d, 3 + k)] = q[:, d, k].astype(np.float32)
        for k in range(7, abi.CP_BODY_FIELDS):
            state[abi.CP_SF_BODY(d, k)] = 0.0
    return state


def state_poses(state):
    """(B, 4, 7) float32 poses (xyz, quat xyzw) of a float32 state SoA."""
    return np.stack([np.stack([state[abi.CP_SF_BODY(d, k)] for k in range(7)], -1) for d in range(4)], 1)


def poses_per_repeat(O, cfg, start, action):
    """(R, B, 4, 7): the poses after each action repeat of one env-step from `start`, from the oracle stepped
    one repeat at a time (the same substeps: a copy of cfg with action_repeats = 1, stepped R times), and the
    oracle's state after the last one."""
    one = abi.cp_config.from_buffer_copy(cfg)
    one.action_repeats = 1
    env = O.Envs(one)
    env.set_state(np.ascontiguousarray(start))
    out = []
    for _ in range(cfg.action_repeats):
        env.step(action)
        out.append(state_poses(env.get_state()))
    return np.stack(out), env.get_state()


def _axes(q):
    x, y, z, w = [q[..., k] for k in range(4)]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], -1),
                     np.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], -1),
                     np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def classify(poses, rc, phys, cam):
    """(..., 4) class of every dynamic body's box for camera `cam`, from poses (..., 4, 7), in float64."""
    p = np.asarray(poses, np.float64)
    eye = np.array([rc.eye[cam][k] for k in range(3)], np.float64)
    f = np.array([rc.target[k] for k in range(3)], np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.array([rc.up[k] for k in range(3)], np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    syk = float(rc.tan_half_fov)
    sxk = syk * rc.width / rc.height
    h = np.array([[phys.half_extents[b + 1][k] for k in range(3)] for b in range(4)], np.float64)
    ax = _axes(p[..., 3:7] / np.linalg.norm(p[..., 3:7], axis=-1, keepdims=True))   # (..., 4, 3 axes, xyz)
    rel = eye - p[..., 0:3]
    inside = (np.abs(np.einsum("...k,...ak->...a", rel, ax)) <= h).all(-1)
    signs = np.array([[(1 if n & 1 else -1), (1 if n & 2 else -1), (1 if n & 4 else -1)] for n in range(8)], np.float64)
    corners = p[..., None, 0:3] + np.einsum("na,...a,...ak->...nk", signs, h, ax)   # (..., 4, 8, 3)
    v = corners - eye
    z = v @ f
    with np.errstate(divide="ignore", invalid="ignore"):
        xs, ys = (v @ r) / (z * sxk), (v @ u) / (z * syk)
    behind = (z < 1e-3).any(-1)
    all_behind = (z < -1e-3).all(-1)
    on = ((np.abs(xs) <= 1.0) & (np.abs(ys) <= 1.0)).all(-1)
    return np.where(inside, EYE_INSIDE,
                    np.where(all_behind, ALL_BEHIND,
                             np.where(behind, STRADDLING, np.where(on, ON_SCREEN, PARTLY_OFF))))


def class_counts(poses, rc, phys):
    """Number of (env, camera, body) triples of poses (B, 4, 7) in each of the five classes."""
    cls = np.stack([classify(poses, rc, phys, c) for c in range(rc.num_cameras)])
    return np.bincount(cls.ravel(), minlength=5)


# (width, height, cameras, repeats, CP_RENDER_V1, the kernel cp_render_kernel_name reports)
KERNELS = [(50, 50, 2, 3, False, "cp_render_small2_kernel"), (50, 50, 1, 1, False, "cp_render_small2_kernel"),
           (37, 23, 2, 1, False, "cp_render_small2_kernel"),
           (50, 50, 2, 3, True, "cp_render_small_kernel"), (50, 50, 1, 1, True, "cp_render_small_kernel"),
           (37, 23, 2, 1, True, "cp_render_small_kernel"),
           (160, 120, 1, 2, False, "cp_render_kernel")]
KERNEL_IDS = [f"{w}x{h}-C{c}R{r}{'-v1' if v1 else ''}" for w, h, c, r, v1, _ in KERNELS]

_EXPECTED = {}


def expected(O, scene, width, height, num_cameras, repeats):
    """The oracle's side of one raster case (cached; the render kernels of one frame size share it): the
    config, the raster config, the reset state, the placed start state, the state after one zero-action
    step, the poses after each repeat and every frame of every env as float16 bits (B, H, W, 3, C, R)."""
    from tests import scene_variants as SV
    key = (scene, width, height, num_cameras, repeats)
    if key not in _EXPECTED:
        cfg = O.default_config(num_envs=B, action_repeats=repeats, initial_force=55.0, seed=11)
        if scene in ("cart", "squat"):          # other box sizes, through cfg.phys
            SV.apply(cfg, scene)
        rc = raster_config(scene, width, height, num_cameras)
        env = O.Envs(abi.cp_config.from_buffer_copy(cfg))
        env.reset()
        reset_state = env.get_state()
        start = place(reset_state.copy(), rc)
        action = np.zeros((B, 2, 2), np.float32)
        poses, end = poses_per_repeat(O, cfg, start, action)
        frames = np.zeros(abi.pixels_shape(B, height, width, num_cameras, repeats), np.uint16)
        for e in range(B):
            for c in range(num_cameras):
                for r in range(repeats):
                    frames[e, :, :, :, c, r] = O.u8_to_f16(O.render_frame(rc, cfg.phys, poses[r, e], c)).view(np.uint16)
        _EXPECTED[key] = dict(cfg=cfg, rc=rc, reset_state=reset_state, start=start, end=end, poses=poses,
                              frames=frames, action=action)
    return _EXPECTED[key]
