"""Scenes off the default one: each variant mutates a cp_config in place (plain module, no fixtures).

The hot kernels are specialised on row structures measured on the scene cp_default_config returns
(c44_ok / c4k_ok / p1_ok / fast_ok, the ez row forms, the settle and bump-phase loops of the reset
kernels); predicates route every other island to the general loops.  The variants below move the
fields those predicates and loops depend on, one group at a time, so that a routing mistake shows as
a parity failure.  tests/test_scene_variants_cpu.py pins on the oracle alone that every variant
stays finite and takes effect; tests/test_gpu_scene_variants.py holds the kernels to the oracle on
them, bit for bit.
"""
import math

import numpy as np

from cartpoleplusplus_amd import abi

G, CART, POLE, CART2, POLE2 = range(5)
CARTS, POLES = (CART, CART2), (POLE, POLE2)

# the run every variant is measured on (both oracle builds finite, nonfinite all zero)
RUN = dict(num_envs=64, action_repeats=2, initial_force=55.0, seed=17, autoreset=1, done_on_bounds=1,
           max_episode_len=70)
RUN_STEPS = 100
ACTION_SEED = 2


def run_actions(steps=RUN_STEPS, B=RUN["num_envs"]):
    """(steps, B, 2) int8: the discrete actions of the measured run."""
    rng = np.random.default_rng(ACTION_SEED)
    return np.stack([rng.integers(0, 5, (B, 2)).astype(np.int8) for _ in range(steps)])


def set_box(phys, body, half_extents=None, mass=None):
    """Half extents and mass of one body together with its solid-box inertia, I_x = m/3 (h_y^2 + h_z^2)
    etc.; inv_inertia is the float32 reciprocal of the float32 inertia (cp_create checks the pair)."""
    if half_extents is not None:
        for k in range(3):
            phys.half_extents[body][k] = half_extents[k]
    if mass is not None:
        phys.inv_mass[body] = 1.0 / mass
    m = 1.0 / float(phys.inv_mass[body])
    h = [float(phys.half_extents[body][k]) for k in range(3)]
    for k in range(3):
        phys.inertia[body][k] = m / 3.0 * (h[(k + 1) % 3] ** 2 + h[(k + 2) % 3] ** 2)
        phys.inv_inertia[body][k] = float(np.float32(1.0) / np.float32(phys.inertia[body][k]))


def default(cfg):
    pass


def gravity(cfg):
    cfg.phys.gravity[0], cfg.phys.gravity[1], cfg.phys.gravity[2] = 0.5, -0.3, -9.81


def moon(cfg):
    cfg.phys.gravity[2] = -1.62


def mass(cfg):
    for b in CARTS:
        set_box(cfg.phys, b, mass=4.0)
    for b in POLES:
        set_box(cfg.phys, b, mass=0.5)


def squat(cfg):
    for b in POLES:
        set_box(cfg.phys, b, half_extents=(0.02, 0.03, 0.15))
        cfg.phys.spawn_pos[b][2] = 0.25


def cart(cfg):
    for b in CARTS:
        set_box(cfg.phys, b, half_extents=(0.15, 0.08, 0.04))
        cfg.phys.spawn_pos[b][2] = 0.095
    for b in POLES:
        cfg.phys.spawn_pos[b][2] = 0.38


def it7(cfg):
    cfg.phys.solver_iterations = 7


def it1(cfg):
    cfg.phys.solver_iterations = 1


def thr0(cfg):
    cfg.phys.residual_threshold = 0.0


def thrbig(cfg):
    cfg.phys.residual_threshold = 1e-3


def erp(cfg):
    cfg.phys.erp = 0.8
    cfg.phys.contact_margin = 0.005
    cfg.phys.warmstart = 0.0


def ws1(cfg):
    cfg.phys.warmstart = 1.0
    cfg.phys.lin_damping = 0.0
    cfg.phys.ang_damping = 0.5


def dt(cfg):
    """The carts tunnel through the ground here; the run stays finite."""
    cfg.phys.dt = 1.0 / 120.0
    cfg.phys.inv_dt = 120.0


def nofric(cfg):
    """No friction rows anywhere."""
    for b in POLES:
        cfg.phys.friction[b] = 0.0


def allfric(cfg):
    for b in range(abi.CP_NUM_BODIES):
        cfg.phys.friction[b] = 0.6


def reset(cfg):
    cfg.settle_steps = 7
    cfg.initial_force_steps = 5
    cfg.action_force = 200.0
    cfg.random_theta = 0


def bounds(cfg):
    cfg.pos_threshold = 0.5
    cfg.angle_threshold = 0.1
    cfg.tan_angle_threshold = math.tan(cfg.angle_threshold)   # of the float32 angle, as cp_create checks
    cfg.sin_angle_threshold = math.sin(cfg.angle_threshold)


def spawn(cfg):
    """cart2 / pole2 close to the first pair, and the pole off centre on its cart."""
    for b in (CART2, POLE2):
        cfg.phys.spawn_pos[b][0] = 0.3
        cfg.phys.spawn_pos[b][1] = 0.08
    cfg.phys.spawn_pos[POLE][0] = 0.06


def edge(cfg):
    cfg.phys.edge_bias = 0.0
    cfg.phys.max_angular_step = 0.01


# solver_iterations = 1 (it1) was added after both oracle builds stayed finite on the measured run
VARIANTS = {f.__name__: f for f in (gravity, moon, mass, squat, cart, it7, it1, thr0, thrbig, erp, ws1, dt, nofric,
                                    allfric, reset, bounds, spawn, edge)}
NAMES = list(VARIANTS)


def apply(cfg, name):
    """cfg with variant `name` applied (in place; returned for convenience)."""
    (default if name == "default" else VARIANTS[name])(cfg)
    return cfg


# ---- the oracle's side of a run, computed once and shared by the tests that compare against it
def drive(env, actions, checkpoints=(), census=None):
    """Step an oracle Envs through `actions` (T, B, ...) and keep everything a parity test compares: per step
    obs, reward, done, terminal obs; at each checkpoint t (steps done so far) the state SoA, the episode
    returns / lengths and the overflow / nonfinite counters.  `merged` sums the merged substeps per env;
    `census` (a contact_census.Census) is fed the state after every step."""
    T = len(actions)
    out = dict(obs=[], reward=[], done=[], term=[], at={}, merged=np.zeros(env.B, np.int64))
    for t in range(T):
        o, r, d, tm = env.step(np.ascontiguousarray(actions[t]), terminal=True)
        out["obs"].append(o)
        out["reward"].append(r)
        out["done"].append(d)
        out["term"].append(tm)
        out["merged"] += env.merged()
        if census is not None:
            census.add(env.get_state())
        if t + 1 in checkpoints or t + 1 == T:
            ret, length = env.episode_returns()
            out["at"][t + 1] = dict(state=env.get_state(), returns=ret, lengths=length, overflow=env.overflow(),
                                    nonfinite=env.nonfinite())
    for k in ("obs", "reward", "done", "term"):
        out[k] = np.stack(out[k])
        out[k].setflags(write=False)
    return out


_RUNS = {}


def variant_config(O, name, precision="f32", **overrides):
    cfg = apply(O.default_config(**{**RUN, **overrides}), name)
    cfg.precision = abi.CP_PRECISION_F64 if precision == "f64" else abi.CP_PRECISION_F32
    return cfg


def variant_run(O, name, precision="f32", **overrides):
    """The measured run of variant `name` on the oracle (cached): its config, actions, reset obs / state and
    drive()'s record with checkpoints after 60 and 100 steps."""
    key = (name, precision, tuple(sorted(overrides.items())))
    if key not in _RUNS:
        cfg = variant_config(O, name, precision, **overrides)
        env = O.Envs(abi.cp_config.from_buffer_copy(cfg), precision=precision)
        actions = run_actions()
        run = dict(cfg=cfg, actions=actions, reset_obs=env.reset(), reset_state=env.get_state(),
                   reset_overflow=env.overflow())
        run.update(drive(env, actions, checkpoints=(60, RUN_STEPS)))
        _RUNS[key] = run
    return _RUNS[key]


# ---- the pile-up: poles thrown against each other (cross-island contacts on every pair, contact-cap overflow)
PILEUP = dict(num_envs=96, action_repeats=3, initial_force=0.0, seed=3)
PILEUP_STEPS = (30, 50)          # [2, 1] pushes, then random discrete actions
PILEUP_CART_FRICTION = (0.0, 0.4)


def pileup_config(cfg, cart_friction):
    for b in CARTS:
        cfg.phys.friction[b] = cart_friction
    return cfg


def _quat_mul(a, b):
    """Hamilton product of xyzw quaternions, arrays (..., 4)."""
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def pileup_place(state):
    """The pile-up placement written into a reset state SoA (float32 or float64, in place), and the actions.

    cart2 and pole2 at x = sep, y = dy; cart2 yawed about z; pole leaning by `tilt` about y (towards +x),
    pole2 yawed and leaning by -tilt (towards the pole).  Values are cast to float32 first, so the fp32
    and fp64 runs start from the same numbers.  Returns the (80, B, 2) int8 actions."""
    B = state.shape[1]
    rng = np.random.default_rng(17)
    sep = rng.uniform(0.22, 0.5, B)
    dy = rng.uniform(-0.05, 0.05, B)
    yaw = rng.uniform(-0.6, 0.6, B)
    tilt = rng.uniform(0.15, 0.5, B)
    zero = np.zeros(B)
    qyaw = np.stack([zero, zero, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], -1)
    qtilt = np.stack([zero, np.sin(0.5 * tilt), zero, np.cos(0.5 * tilt)], -1)
    qtilt_neg = qtilt * np.array([1.0, -1.0, 1.0, 1.0])

    def f32(x):
        return np.asarray(x, np.float64).astype(np.float32)

    for d in (2, 3):                                      # dynamic ids of cart2, pole2
        state[abi.CP_SF_BODY(d, 0)] = f32(sep)
        state[abi.CP_SF_BODY(d, 1)] = f32(dy)
    for d, q in ((2, qyaw), (1, qtilt), (3, _quat_mul(qyaw, qtilt_neg))):
        for k in range(4):
            state[abi.CP_SF_BODY(d, 3 + k)] = f32(q[:, k])
    n_push, n_rand = PILEUP_STEPS
    acts = [np.tile(np.array([2, 1], np.int8), (B, 1)) for _ in range(n_push)]   # cart +x, cart2 -x
    acts += [rng.integers(0, 5, (B, 2)).astype(np.int8) for _ in range(n_rand)]
    return np.stack(acts)


def pileup_run(O, cart_friction, precision="f32"):
    """The pile-up on the oracle (cached): config, the placed start state, the actions, drive()'s record and the
    contact census of every step end."""
    from tests.contact_census import Census
    key = ("pileup", cart_friction, precision)
    if key not in _RUNS:
        cfg = pileup_config(O.default_config(**PILEUP), cart_friction)
        cfg.precision = abi.CP_PRECISION_F64 if precision == "f64" else abi.CP_PRECISION_F32
        env = O.Envs(abi.cp_config.from_buffer_copy(cfg), precision=precision)
        env.reset()
        start = env.get_state()
        actions = pileup_place(start)
        env.set_state(start)
        census = Census(env.B)
        run = dict(cfg=cfg, start=start, actions=actions, census=census, reset_overflow=env.overflow())
        run.update(drive(env, actions, census=census))
        _RUNS[key] = run
    return _RUNS[key]
