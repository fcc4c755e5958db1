"""HIP kernel (through the C-ABI) vs the CPU oracle, same config, same inputs.

The kernel and the fp32 oracle perform the same fp32 operations in the same order
(explicit fma, -ffp-contract=off on both sides, own transcendentals), so the bar is
bit-exact equality (raw bits: a signed-zero difference fails) of obs / reward / done /
full state.  Every case runs on both register budgets of the step and autoreset kernels
(SHAPES: cp_set_kernel_shape), so the throughput shape that bench.py times at 65,536 envs
is under the same bar as the latency shape and its WIDE layout, which small batches pick by default.  Full-size
(B = 65,536) runs are checked on a random subset of envs plus size-independent properties.
"""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native
from cartpoleplusplus_amd.batched import BatchedCartpole

pytestmark = pytest.mark.gpu


# (step kernel shape, autoreset kernel shape): the combinations of the two register budgets, and the WIDE
# layout of the latency budget (16 lanes per env, round 6) as step kernel, reset kernel and both
SHAPES = [("throughput", "throughput"), ("latency", "latency"), ("throughput", "latency"),
          ("latency", "throughput"), ("wide", "wide"), ("throughput", "wide"), ("wide", "latency"),
          ("wide8", "wide8"), ("wide", "wide64"), ("throughput", "list")]
SHAPE_IDS = ["tp-tp", "lat-lat", "tp-lat", "lat-tp", "wide-wide", "tp-wide", "wide-lat", "wide8-wide8", "wide-wide64",
             "tp-list"]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)


def _pair(O, shape=None, mutate=None, precision="f32", oracle=True, **kw):
    """A GPU handle and an oracle Envs on one config: the defaults, the overrides **kw, then mutate(cfg) (a
    scene variant of tests/scene_variants.py).  oracle=False: the handle alone (the oracle's side of the run
    is a recorded one, shared between cases)."""
    cfg = native.default_config(**kw)
    if mutate is not None:
        mutate(cfg)
    if precision == "f64":
        cfg.precision = abi.CP_PRECISION_F64
    gpu = BatchedCartpole(cfg.num_envs, 0, config=abi.cp_config.from_buffer_copy(cfg))
    if shape is not None:
        gpu.set_kernel_shape(*shape)
        assert gpu.kernel_shape() == tuple(shape)
    orc = O.Envs(abi.cp_config.from_buffer_copy(cfg), precision=precision) if oracle else None
    return gpu, orc


def _np(t):
    return t.detach().cpu().numpy()


def _assert_same(a, b, what):
    """Bit-exact: float32 arrays are compared as their uint32 bits (-0.0 != +0.0); a NaN must be a
    NaN on both sides (its payload is the hardware's default NaN: gfx950 and x86 differ)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        na, nb = np.isnan(a), np.isnan(b)
        ua = np.where(na, np.uint32(0x7FC00000), np.ascontiguousarray(a).view(np.uint32))
        ub = np.where(nb, np.uint32(0x7FC00000), np.ascontiguousarray(b).view(np.uint32))
        same = np.array_equal(ua, ub)
    else:
        same = np.array_equal(a, b, equal_nan=True)
    if not same:
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        idx = np.unravel_index(np.nanargmax(d), d.shape)
        if a.dtype == b.dtype == np.float32:
            diff = ua != ub
        else:
            diff = d != 0
        where = [tuple(int(x) for x in w) for w in np.argwhere(diff)[:6]]
        vals = [(float(a[w]), float(b[w])) for w in where]
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ, max |diff| {np.nanmax(d):.3e} at {idx}; "
                             f"first {where} (gpu, oracle) {vals}")


def _compare_state(gpu, orc, what):
    _assert_same(_np(gpu.get_state()), orc.get_state(), what + " state")


@shapes
def test_reset_philox_bitexact(oracle_mod, shape):
    gpu, orc = _pair(oracle_mod, shape, num_envs=200, action_repeats=3, initial_force=55.0, seed=1234)
    _assert_same(_np(gpu.reset()), orc.reset(), "reset obs")
    _compare_state(gpu, orc, "reset")
    _assert_same(_np(gpu.overflow_counts()), np.zeros(200, np.int32), "overflow")


@shapes
@pytest.mark.parametrize("R,S", [(3, 1), (2, 1), (3, 4)])
def test_continuous_random_actions_200_steps(oracle_mod, R, S, shape):
    B = 96
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=R, steps_per_repeat=S, initial_force=55.0, seed=7)
    _assert_same(_np(gpu.reset()), orc.reset(), "reset obs")
    rng = np.random.default_rng(123)
    for t in range(200):
        a = rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)
        go, gr, gd = gpu.step(torch.from_numpy(a).cuda())
        oo, orw, od = orc.step(a)
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gr), orw, f"reward step {t}")
        _assert_same(_np(gd), od, f"done step {t}")
    _compare_state(gpu, orc, "after 200 steps")
    assert _np(gd).all()   # max_episode_len = 200


@shapes
def test_discrete_autoreset_bounds(oracle_mod, shape):
    B = 130
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=3, initial_force=55.0, seed=99, autoreset=1,
                     done_on_bounds=1, max_episode_len=40)
    _assert_same(_np(gpu.reset()), orc.reset(), "reset")
    rng = np.random.default_rng(5)
    for t in range(120):
        a = rng.integers(0, 5, (B, 2)).astype(np.int8)
        go, gr, gd = gpu.step(torch.from_numpy(a).cuda())
        oo, orw, od, ot = orc.step(a, terminal=True)
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gd), od, f"done step {t}")
        done = od.astype(bool)
        _assert_same(_np(gpu.terminal_obs)[done], ot[done], f"terminal obs step {t}")
    _compare_state(gpu, orc, "autoreset")
    gr_, gl_ = gpu.episode_returns()
    orr, orl = orc.episode_returns()
    _assert_same(_np(gr_), orr, "episode returns")
    _assert_same(_np(gl_), orl, "episode lengths")
    assert (orl > 0).all() and (orl <= 40).all()


@shapes
def test_host_bump_mode(oracle_mod, shape):
    B = 33
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=2, bump_mode=abi.CP_BUMP_HOST)
    rng = np.random.default_rng(0)
    f = rng.uniform(-200, 200, (B, 30, 2, 2)).astype(np.float32)
    gpu.set_bump_forces(torch.from_numpy(f).cuda())
    orc.set_bump_forces(f)
    _assert_same(_np(gpu.reset()), orc.reset(), "reset obs")
    for t in range(30):
        a = rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)
        go, _, _ = gpu.step(torch.from_numpy(a).cuda())
        oo, _, _ = orc.step(a)
        _assert_same(_np(go), oo, f"obs step {t}")


@shapes
@pytest.mark.parametrize("bug", [True, False])
def test_readback_12_state(oracle_mod, bug, shape):
    B, R, S = 40, 3, 2
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=R, steps_per_repeat=S, initial_force=55.0, seed=3)
    gpu.enable_readback(True, reference_bug=bug)
    gpu.reset()
    orc.reset()
    rng = np.random.default_rng(1)
    for t in range(25):
        a = rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)
        gpu.step(torch.from_numpy(a).cuda())
        _, _, _, rb = orc.step(a, readback=True, readback_bug=bug)
        _assert_same(_np(gpu.readback), rb, f"readback step {t}")
    if bug:   # bullet_cartpole.py:224 reads pole's velocity into pole2's rows
        r = _np(gpu.readback)
        assert np.array_equal(r[:, 1, :, :, 2:4], r[:, 0, :, :, 2:4])


@shapes
def test_step_after_done_and_mask_reset(oracle_mod, shape):
    B = 64
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=2, max_episode_len=3, seed=11, initial_force=55.0)
    gpu.reset()
    orc.reset()
    a = np.zeros((B, 2, 2), np.float32)
    for t in range(5):   # steps 4 and 5 are after done
        go, gr, gd = gpu.step(torch.from_numpy(a).cuda())
        oo, orw, od = orc.step(a)
        _assert_same(_np(go), oo, f"obs {t}")
        _assert_same(_np(gr), orw, f"reward {t}")
        _assert_same(_np(gd), od, f"done {t}")
    assert (_np(gr) == 0).all() and (_np(gd) == 1).all()
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    gpu.reset(torch.from_numpy(mask).cuda())
    orc_obs = np.zeros((B, 2, 2, 7), np.float32)
    orc_obs[:] = _np(gpu.obs)          # unmasked rows are left untouched by both
    orc.reset(mask, obs=orc_obs)
    _assert_same(_np(gpu.obs), orc_obs, "masked reset obs")
    _compare_state(gpu, orc, "masked reset")


@shapes
def test_state_roundtrip_into_oracle(oracle_mod, shape):
    B = 50
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=3, initial_force=200.0, seed=5)
    gpu.reset()
    rng = np.random.default_rng(2)
    for _ in range(20):
        gpu.step(torch.from_numpy(rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)).cuda())
    orc.set_state(_np(gpu.get_state()))
    gpu2 = BatchedCartpole(B, 0, config=abi.cp_config.from_buffer_copy(gpu.cfg))
    other = shape[::-1] if shape[1] not in ("wide64", "list") else ("latency", "wide")   # (reset layouts only)
    gpu2.set_kernel_shape(*other)   # the copy runs the other shapes
    gpu2.set_state(gpu.get_state())
    for t in range(10):
        a = rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)
        g1, _, _ = gpu.step(torch.from_numpy(a).cuda())
        g2, _, _ = gpu2.step(torch.from_numpy(a).cuda())
        oo, _, _ = orc.step(a)
        _assert_same(_np(g1), oo, f"obs {t}")
        _assert_same(_np(g2), oo, f"obs (set_state copy) {t}")


@shapes
def test_cross_island_contact_merged_solve(oracle_mod, shape):
    """The merged path: cart2 + pole2 placed against cart + pole (gap 0-3 cm, yaw up to
    0.6 rad, y offset up to 15 cm) and the carts pushed into each other, then random pushes.
    The cross pairs 5-8 touch, so the oracle solves those envs merged (one group, pair order
    0 2 1 3 4 9 5 6 7 8; DPP whole-env view in the kernels, cp_physics.h cross_view), and the
    GPU must stay bit-exact through it on both kernel shapes."""
    B = 96
    gpu, orc = _pair(oracle_mod, shape, num_envs=B, action_repeats=3, initial_force=0.0, seed=3)
    gpu.reset()
    orc.reset()
    st = orc.get_state()
    _assert_same(_np(gpu.get_state()), st, "reset state")
    rng = np.random.default_rng(17)
    gap = rng.uniform(0.0, 0.03, B)
    yaw = rng.uniform(-0.6, 0.6, B)
    dy = rng.uniform(-0.15, 0.15, B)
    for d in (2, 3):                                   # cart2, pole2
        st[abi.CP_SF_BODY(d, 0)] = (0.2 + gap).astype(np.float32)
        st[abi.CP_SF_BODY(d, 1)] = dy.astype(np.float32)
        st[abi.CP_SF_BODY(d, 5)] = np.sin(0.5 * yaw).astype(np.float32)
        st[abi.CP_SF_BODY(d, 6)] = np.cos(0.5 * yaw).astype(np.float32)
    orc.set_state(st)
    gpu.set_state(torch.from_numpy(st).cuda())
    merged = np.zeros(B, np.int64)
    for t in range(80):
        if t < 40:                                     # cart +x, cart2 -x (discrete table 2 / 1)
            a = np.tile(np.array([2, 1], np.int8), (B, 1))
        else:
            a = rng.integers(0, 5, (B, 2)).astype(np.int8)
        go, gr, gd = gpu.step(torch.from_numpy(a).cuda())
        oo, orw, od = orc.step(a)
        merged += orc.merged()
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gd), od, f"done step {t}")
    _compare_state(gpu, orc, "after the merged rollout")
    _assert_same(_np(gpu.overflow_counts()), orc.overflow(), "overflow after the merged rollout")
    assert (merged > 0).sum() >= B * 3 // 4, f"only {(merged > 0).sum()} envs ran a merged solve"
    assert merged.sum() >= 30 * B


def test_full_size_c2_200_steps(oracle_mod):
    """BASELINE configs[1] (C2) at its full size: 4,096 envs, continuous U[-1,1] actions (bench.py's
    hashed stream), R = 3, F_init 55, seed 1234, 200 steps from reset on the kernel shapes bench.py
    times at this size (cp_create's choice), every env bit-exact against the oracle."""
    import os

    import bench
    B = 4096
    gpu, orc = _pair(oracle_mod, None, num_envs=B, action_repeats=3, initial_force=55.0, seed=bench.SEED)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    _assert_same(_np(gpu.reset()), orc.reset(), "reset obs")
    acts = bench.make_actions(True, B, 0, 200, bench.SEED, gpu.device)
    rew = np.zeros(B, np.float32)
    done = np.zeros(B, np.uint8)
    for t in range(200):
        go, gr, gd = gpu.step(acts[t])
        oo = np.zeros((B, 3, 2, 7), np.float32)
        orc.step_omp(np.ascontiguousarray(_np(acts[t])), abi.CP_ACTION_CONTINUOUS, oo, rew, done, threads)
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gd), done, f"done step {t}")
    _compare_state(gpu, orc, "C2 after 200 steps")
    assert done.all()


def test_full_size_bench_config_subset_parity_and_properties(oracle_mod):
    """B = 65,536, discrete, R = 3, autoreset (BASELINE config 3): the whole batch is checked
    for finiteness, unit quaternions and run-to-run determinism; then every env's step
    counter is set to 198 (cp_set_state), so the second step after that ends all 65,536
    episodes at once (bullet_cartpole.py:255-257) and the burst runs through the step
    kernel's ballot-compacted reset list and the throughput-shaped reset kernel.  Four
    blocks of 128 envs (env ids keep the Philox bump streams) are re-simulated on the oracle
    from the GPU state across the burst: obs, terminal obs, done, bit for bit."""
    B = 65536
    cfg = native.default_config(num_envs=B, action_repeats=3, initial_force=55.0, seed=1234, autoreset=1)
    g1 = BatchedCartpole(B, 0, config=abi.cp_config.from_buffer_copy(cfg))
    g2 = BatchedCartpole(B, 0, config=abi.cp_config.from_buffer_copy(cfg))
    assert g1.kernel_shape() == ("throughput", "throughput")   # what bench.py times at C3
    g1.reset()
    g2.reset()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    for t in range(12):
        a = torch.randint(0, 5, (B, 2), device="cuda", generator=gen, dtype=torch.int8)
        o1, _, _ = g1.step(a)
        o2, _, _ = g2.step(a)
    assert torch.equal(o1, o2)                                  # deterministic
    assert torch.isfinite(o1).all()
    q = o1[..., 3:7].double()
    assert torch.allclose(q.norm(dim=-1), torch.ones_like(q[..., 0]), atol=1e-5)
    st = _np(g1.get_state())
    st.view(np.int32)[abi.CP_SF_STEPS] = 198
    g1.set_state(torch.from_numpy(st).cuda())
    blocks = [0, 20000, 40960, B - 128]
    orcs = []
    for lo in blocks:
        sub = abi.cp_config.from_buffer_copy(cfg)
        sub.num_envs, sub.env_id_offset = 128, lo
        orc = oracle_mod.Envs(sub)
        orc.set_state(np.ascontiguousarray(st[:, lo:lo + 128]))
        orcs.append(orc)
    rng = np.random.default_rng(9)
    for t in range(5):
        a = rng.integers(0, 5, (B, 2)).astype(np.int8)
        go, gr, gd = g1.step(torch.from_numpy(a).cuda())
        go, gd, gt = _np(go), _np(gd), _np(g1.terminal_obs)
        if t == 1:
            assert gd.all(), "every episode ends at step 200"
        for lo, orc in zip(blocks, orcs):
            oo, orw, od, ot = orc.step(np.ascontiguousarray(a[lo:lo + 128]), terminal=True)
            _assert_same(go[lo:lo + 128], oo, f"block {lo} obs {t}")
            _assert_same(gd[lo:lo + 128], od, f"block {lo} done {t}")
            if t == 1:
                _assert_same(gt[lo:lo + 128], ot, f"block {lo} terminal obs")
    eps = _np(g1.get_state()).view(np.int32)[abi.CP_SF_EPISODE]
    assert (eps == 2).all()                                     # reset once, auto-reset once


def test_gym_mirror_matches_oracle_and_reference_errors(oracle_mod):
    from cartpoleplusplus_amd.bullet_cartpole import BulletCartpole, add_opts, draw_bump_forces
    ap = argparse.ArgumentParser()
    add_opts(ap)
    opts = ap.parse_args(["--initial-force", "55", "--action-repeats", "3"])
    env = BulletCartpole(opts, discrete_actions=False)
    with pytest.raises(AttributeError):
        env.step(np.zeros((2, 2)))         # step before reset (reference: self.done unset)
    np.random.seed(0)
    obs = env.reset()
    assert obs.shape == (3, 2, 7) and obs.dtype == np.float32
    cfg = oracle_mod.default_config(num_envs=1, action_repeats=3, initial_force=55.0, bump_mode=abi.CP_BUMP_HOST)
    orc = oracle_mod.Envs(cfg)
    np.random.seed(0)
    orc.set_bump_forces(draw_bump_forces(55.0, True)[None].astype(np.float32))
    _assert_same(obs, orc.reset()[0], "mirror reset")
    with pytest.raises(IndexError):
        env.step(np.zeros((1, 2)))         # declared Box(1,2) action: the fork indexes action[1]
    with pytest.raises(TypeError):
        env.step(3)
    a = np.array([[0.5, -0.25], [-1.0, 0.75]])
    o, r, d, info = env.step(a)
    oo, _, _ = orc.step(a.astype(np.float32).reshape(1, 2, 2))
    _assert_same(o, oo[0], "mirror step")
    assert r == 1.0 and d is False and info == {}
    assert env.monkey_positions.shape == (2, 3, 1, 2, 3) and env.monkey_velocities.shape == (2, 3, 1, 2, 3)
    denv = BulletCartpole(opts, discrete_actions=True)
    assert denv.action_space.n == 5
    np.random.seed(1)
    denv.reset()
    with pytest.raises(TypeError):
        denv.step(2)                        # reference: 'int' object is not subscriptable
    denv.step([1, 4])


@pytest.mark.parametrize("io", ["zero_copy", "graph", "eager", "mixed"])
def test_gym_mirror_discrete_c1_vs_oracle(oracle_mod, io):
    """C1's configuration through the reference's surface: B = 1, R = 2 (the reference default),
    F_init 55, discrete actions, two episodes of 200 steps with the reference's own reset loop
    (the agent calls reset() after done); obs and the 12-state readback (monkey_positions /
    velocities, the :224 bug included) bit-exact against the oracle, with the step as one launch over
    mapped pinned host buffers (the default), replayed as a hipGraph, eagerly, and switching between
    the three every few steps (the readback pointer follows the path)."""
    from cartpoleplusplus_amd.bullet_cartpole import BulletCartpole, add_opts, draw_bump_forces
    ap = argparse.ArgumentParser()
    add_opts(ap)
    opts = ap.parse_args(["--initial-force", "55"])
    env = BulletCartpole(opts, discrete_actions=True)
    assert env.step_io == "zero_copy"
    ios = ["zero_copy", "graph", "eager"]
    if io != "mixed":
        env.step_io = io
    cfg = oracle_mod.default_config(num_envs=1, action_repeats=2, initial_force=55.0, bump_mode=abi.CP_BUMP_HOST)
    orc = oracle_mod.Envs(cfg)
    rng = np.random.default_rng(21)
    for ep in range(2):
        np.random.seed(100 + ep)
        obs = env.reset()
        np.random.seed(100 + ep)
        orc.set_bump_forces(draw_bump_forces(55.0, True)[None].astype(np.float32))
        _assert_same(obs, orc.reset()[0], f"episode {ep} reset")
        done, t = False, 0
        while not done:
            a = rng.integers(0, 5, 2)
            if io == "mixed":
                env.step_io = ios[(t // 7) % 3]
            o, r, done, info = env.step(a)
            oo, _, od, rb = orc.step(a.astype(np.int8).reshape(1, 2), readback=True, readback_bug=True)
            _assert_same(o, oo[0], f"episode {ep} step {t} obs")
            _assert_same(env.monkey_positions.astype(np.float32), rb[0][..., 0:2, :], f"episode {ep} step {t} positions")
            _assert_same(env.monkey_velocities.astype(np.float32), rb[0][..., 2:4, :], f"step {t} velocities")
            t += 1
        assert t == 200 and info == {"done_reason": "episode length"}


def test_batched_rejects_wrong_buffers_before_the_abi():
    """Shapes / dtypes the C-ABI would read blindly raise ValueError, and the
    handle stays usable afterwards."""
    env = BatchedCartpole(16, 0, action_repeats=2, autoreset=True)
    env.reset()
    with pytest.raises(ValueError):
        env.step(torch.zeros((16, 2), device="cuda"))                   # float (B,2): not a continuous action
    with pytest.raises(ValueError):
        env.step(torch.zeros((8, 2), dtype=torch.int8, device="cuda"))  # short batch
    with pytest.raises(ValueError):
        env.step(torch.zeros((16, 2, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.reset(mask=torch.ones(15, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        env.set_bump_forces(torch.zeros((16, 29, 2, 2), device="cuda"))
    with pytest.raises(ValueError):
        env.set_state(torch.zeros((abi.CP_STATE_FIELDS, 15), device="cuda"))
    o, r, d = env.step(torch.zeros((16, 2), dtype=torch.int8, device="cuda"))
    assert torch.isfinite(o).all() and (r == 1).all()


@shapes
def test_cart_friction_config(oracle_mod, shape):
    """A non-default scene: the carts get friction (the reference's cart.urdf has mu = 0), so the
    ground-cart and cart-pole pairs carry friction rows, which the reset kernels' settle and bump-phase
    loops do not run (c44_ok / c4k_ok must route such islands to the general loop)."""
    B = 96
    cfg = native.default_config(num_envs=B, action_repeats=2, initial_force=55.0, seed=17, autoreset=1,
                                done_on_bounds=1, max_episode_len=30)
    cfg.phys.friction[abi.CP_BODY_CART] = 0.3
    cfg.phys.friction[abi.CP_BODY_CART2] = 0.3
    gpu = BatchedCartpole(B, 0, config=abi.cp_config.from_buffer_copy(cfg))
    gpu.set_kernel_shape(*shape)
    orc = oracle_mod.Envs(abi.cp_config.from_buffer_copy(cfg))
    _assert_same(_np(gpu.reset()), orc.reset(), "reset")
    _compare_state(gpu, orc, "reset")
    # ground-cart and cart-pole ask for 8 friction rows of the island's 5: the reset already drops rows
    assert orc.overflow().all()
    _assert_same(_np(gpu.overflow_counts()), orc.overflow(), "overflow after the reset")
    rng = np.random.default_rng(2)
    for t in range(70):
        a = rng.integers(0, 5, (B, 2)).astype(np.int8)
        go, gr, gd = gpu.step(torch.from_numpy(a).cuda())
        oo, orw, od = orc.step(a)
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gd), od, f"done step {t}")
    _compare_state(gpu, orc, "after 70 steps")
    _assert_same(_np(gpu.overflow_counts()), orc.overflow(), "overflow after 70 steps")


def test_auto_shapes_by_batch_size():
    """CP_SHAPE_AUTO: the widest latency layout whose waves fit the chip once (16
    lanes per env up to 4,096 envs, 8 up to 8,192, two up to 32,768; the reset kernel one env per wave up
    to 1,024 envs), the throughput shape above; the reset list of bounds-terminated episodes one env per
    wave up to 1,024 envs by the list's own length (CP_SHAPE_LIST); fp64 and the model switches on the two-lane
    latency layout."""
    def shapes(B, **kw):
        env = BatchedCartpole(B, 0, **kw)
        s = env.kernel_shape()
        env.close()
        return s
    assert shapes(1) == ("wide", "wide64")
    assert shapes(1024, autoreset=True) == ("wide", "wide64")
    assert shapes(4096, autoreset=True) == ("wide", "wide")
    assert shapes(8192, autoreset=True) == ("wide8", "wide8")
    assert shapes(16384, autoreset=True) == ("latency", "latency")
    assert shapes(65536, autoreset=True) == ("throughput", "throughput")
    assert shapes(65536, autoreset=True, done_on_bounds=True) == ("throughput", "list")
    # NEXT_STEP: the same by the list's length; fixed-length episodes keep the two-lane reset beside the step
    assert shapes(65536, autoreset="next_step", done_on_bounds=True) == ("throughput", "list")
    assert shapes(4096, autoreset="next_step") == ("wide", "latency")
    assert shapes(64, precision="f64") == ("latency", "latency")
    assert shapes(64, model_flags=abi.CP_MODEL_SLEEPING) == ("latency", "latency")


@pytest.mark.parametrize("B", [8192, 33000])
def test_reset_list_tiers_by_length(oracle_mod, B):
    """CP_SHAPE_LIST (the reset shape of bounds-terminated handles): one launch per layout, and the list's
    length picks the one that runs -- one env per wave up to 1,024 envs, 16 lanes up to 4,096, the two-lane
    latency layout up to 32,768, the throughput shape above.  Masked resets on both sides of every tier
    boundary on one handle, then lists made by the step kernel itself, bit-exact against the oracle (obs and
    the whole state SoA).  33,000 envs: the full reset is the throughput tier's (the oracle resets serially)."""
    gpu, orc = _pair(oracle_mod, ("throughput", "list"), num_envs=B, action_repeats=3, initial_force=55.0,
                     seed=99, done_on_bounds=1, autoreset=1)
    _assert_same(_np(gpu.reset()), orc.reset(), "full reset")   # B envs: the latency or throughput tier
    _compare_state(gpu, orc, "full reset")
    rng = np.random.default_rng(B)
    for n in ((1, 1024, 1025, 4096, 4097, B) if B <= 32768 else ()):
        mask = np.zeros(B, np.uint8)
        mask[rng.choice(B, n, replace=False)] = 1
        gpu.reset(torch.from_numpy(mask).cuda())
        orc_obs = _np(gpu.obs).copy()   # unmasked rows are left untouched by both
        orc.reset(mask, obs=orc_obs)
        _assert_same(_np(gpu.obs), orc_obs, f"reset of {n} envs obs")
        _compare_state(gpu, orc, f"reset of {n} envs")
    T = 30 if B <= 32768 else 4
    a = rng.integers(0, 5, (T, B, 2)).astype(np.int8)
    for t in range(T):   # lists made by the step kernel (bounds termination), through the same launches
        go, gr, gd = gpu.step(torch.from_numpy(a[t]).cuda())
        oo, orw, od = orc.step(a[t])
        _assert_same(_np(go), oo, f"obs step {t}")
        _assert_same(_np(gd), od, f"done step {t}")
    _compare_state(gpu, orc, f"after {T} steps")
