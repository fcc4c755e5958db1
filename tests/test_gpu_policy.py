"""MLP policy kernel on the MI355X (cp_set_policy, cp_policy_act): the actions against the numpy
restatement (tests/policy_ref.py; bit-exact wherever the contract fixes every rounding), done envs, live
weights, the rejections, and cp_step / cp_rollout unchanged with a policy set."""
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native
from cartpoleplusplus_amd.batched import BatchedCartpole
from tests import policy_ref as ref
from tests.test_gpu_parity import _assert_same, _np

pytestmark = pytest.mark.gpu


def _env(shape=None, **kw):
    kw.setdefault("initial_force", 55.0)
    cfg = native.default_config(**kw)
    env = BatchedCartpole(cfg.num_envs, 0, config=abi.cp_config.from_buffer_copy(cfg))
    if shape is not None:
        env.set_kernel_shape(shape, shape)
    return env


def _t(layers):
    return [(torch.from_numpy(W), torch.from_numpy(b)) for W, b in layers]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same(a, b, what):
    """Raw bits (a NaN payload included: both sides are the same GPU)."""
    assert np.array_equal(_bits(_np(a)), _bits(_np(b))), what


_REF_OBS = {}


def _obs_after_reset(B, R):
    """A handle of B envs, reset (obs of every env differ: random bump directions), shared per (B, R)."""
    if (B, R) not in _REF_OBS:
        env = _env(num_envs=B, action_repeats=R, seed=11)
        env.reset()
        for _ in range(2):   # off the reset pose: every repeat row differs
            env.step(torch.from_numpy(np.random.default_rng(B).integers(0, 5, (B, 2)).astype(np.int8)).cuda())
        _REF_OBS[(B, R)] = env
    return _REF_OBS[(B, R)]


@pytest.mark.parametrize("B", [3, 33, 128])
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("head", ["clip", "argmax"])
def test_policy_act_bit_exact(head, R, B):
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(100 * R + B)
    layers = ref.random_layers(rng, (14 * R, 7, 5, 4 if head == "clip" else 10), scale=2.0)
    env.set_policy(_t(layers), head)
    x = _np(env.obs).reshape(B, -1)
    z = ref.forward(layers, x)
    if head == "clip":
        noise = rng.uniform(-0.5, 0.5, (B, 2, 2)).astype(np.float32)
        _assert_same(_np(env.policy_act(noise=torch.from_numpy(noise))), ref.act_clip(z, noise), "clip + noise")
        _assert_same(_np(env.policy_act()), ref.act_clip(z), "clip, no noise")
    else:
        _assert_same(_np(env.policy_act()), ref.act_argmax(z), "argmax")
    env.set_policy(None)


@pytest.mark.parametrize("head", ["clip", "argmax"])
def test_policy_act_bit_exact_wide_layers(head):
    B, R = 33, 3
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(7)
    layers = ref.random_layers(rng, (14 * R, 100, 100, 50, 4 if head == "clip" else 10), scale=1.5)
    env.set_policy(_t(layers), head)
    z = ref.forward(layers, _np(env.obs).reshape(B, -1))
    if head == "clip":
        noise = rng.uniform(-0.5, 0.5, (B, 2, 2)).astype(np.float32)
        _assert_same(_np(env.policy_act(noise=torch.from_numpy(noise))), ref.act_clip(z, noise), "clip + noise")
    else:
        _assert_same(_np(env.policy_act()), ref.act_argmax(z), "argmax")
    env.set_policy(None)


@pytest.mark.parametrize("R,B", [(1, 33), (3, 128)])
def test_policy_act_tanh(R, B):
    """The pre-activation z is exact in the restatement; tanhf is OCML's (OpenCL: <= 5 ulp, and one fp32 ulp
    in [-1, 1] is <= 6e-8, so 3e-7), hence |a - float32(tanh64(z))| <= 1e-6."""
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(R)
    layers = ref.random_layers(rng, (14 * R, 7, 5, 4), scale=6.0)   # |z| from ~0 to a few: tanh's whole bend
    env.set_policy(_t(layers), "tanh")
    z = ref.forward(layers, _np(env.obs).reshape(B, -1))
    a = _np(env.policy_act()).reshape(B, 4)
    exp = np.tanh(z.astype(np.float64)).astype(np.float32)
    err = np.abs(a.astype(np.float64) - exp.astype(np.float64)).max()
    print(f"tanh head: max |a - tanh64(z)| = {err:.3g}, |z| up to {np.abs(z).max():.3g}")
    assert err <= 1e-6
    assert np.abs(z).max() > 0.5 and np.abs(a).max() <= 1.0
    # with noise the clip acts on tanhf(z) + n
    noise = rng.uniform(-1.0, 1.0, (B, 2, 2)).astype(np.float32)
    an = _np(env.policy_act(noise=torch.from_numpy(noise))).reshape(B, 4)
    expn = np.clip(np.tanh(z.astype(np.float64)) + noise.reshape(B, 4), -1.0, 1.0)
    assert np.abs(an - expn).max() <= 1e-6
    env.set_policy(None)


def test_policy_act_sample():
    """epsilon = 0.25: the epsilon draws and their actions are exact; every other draw lies in its float64
    softmax interval widened by delta = 2^-18 (five positive terms, each a few ulp of expf error plus one
    rounding per add: below 2^-20; delta is four times that)."""
    B, R, eps, seed = 128, 3, 0.25, (3 << 32) | 77
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(5)
    layers = ref.random_layers(rng, (14 * R, 7, 5, 10), scale=2.0)
    env.set_policy(_t(layers), "sample", epsilon=eps, seed=seed)
    z = ref.forward(layers, _np(env.obs).reshape(B, -1))
    base = _np(env.get_state())
    counts = np.zeros(5, np.int64)
    n_eps = n_soft = 0
    for rep in range(6):   # other counters: other Philox counters, so other draws from the same logits
        st = base.copy()
        ints = abi.state_ints(st)
        ints[abi.CP_SF_STEPS] = rng.integers(0, 150, B)
        ints[abi.CP_SF_EPISODE] = rng.integers(0, 1 << 20, B)
        env.set_state(torch.from_numpy(st))
        a = _np(env.policy_act())
        assert a.dtype == np.int8 and a.shape == (B, 2) and a.min() >= 0 and a.max() <= 4
        w = ref.sample_words(ints[abi.CP_SF_STEPS], ints[abi.CP_SF_EPISODE], np.arange(B), seed)
        ne, ns, near = ref.check_sample(z, a, w, eps)
        assert near < 0.01, "the reference itself is too often within delta of a boundary"
        n_eps, n_soft = n_eps + ne, n_soft + ns
        counts += np.bincount(a.reshape(-1), minlength=5)
    env.set_state(torch.from_numpy(base))
    env.set_policy(None)
    print(f"sample head: {n_eps} epsilon draws, {n_soft} softmax draws, actions {counts.tolist()}")
    assert (counts > 0).all()
    assert 0.15 < n_eps / (n_eps + n_soft) < 0.35


@pytest.mark.parametrize("head", ["clip", "sample"])
def test_done_envs_get_zero_actions(head):
    """An env that is done is not evaluated: its actions_out entry is 0 (both action kinds); the other envs
    get the restatement's values.  Done envs come from stepping a no-autoreset handle past its episode
    length (envs start at different step counters) and from a done field set through set_state."""
    B, R, eps, seed = 33, 2, 0.25, 5
    env = _env(num_envs=B, action_repeats=R, seed=3, autoreset=0, max_episode_len=6)
    env.reset()
    st = _np(env.get_state())
    abi.state_ints(st)[abi.CP_SF_STEPS][::3] = 4          # these finish after 2 steps
    abi.state_ints(st)[abi.CP_SF_DONE][5] = 1             # done from the start
    env.set_state(torch.from_numpy(st))
    rng = np.random.default_rng(21)
    layers = ref.random_layers(rng, (14 * R, 7, 5, 4 if head == "clip" else 10), scale=2.0)
    env.set_policy(_t(layers), head, epsilon=eps, seed=seed)
    noise = torch.from_numpy(rng.uniform(0.3, 0.5, (B, 2, 2)).astype(np.float32)) if head == "clip" else None
    seen = 0
    for k in range(4):
        ints = abi.state_ints(_np(env.get_state()))
        done = ints[abi.CP_SF_DONE] != 0
        a = _np(env.policy_act(noise=noise))
        assert not a[done].any(), f"step {k}: a done env's action is 0"
        z = ref.forward(layers, _np(env.obs).reshape(B, -1))
        if head == "clip":      # the noise alone keeps every evaluated action off 0
            _assert_same(a[~done], ref.act_clip(z, _np(noise))[~done], f"step {k}: live envs")
            assert np.abs(a[~done]).min() > 0
        else:
            w = ref.sample_words(ints[abi.CP_SF_STEPS], ints[abi.CP_SF_EPISODE], np.arange(B), seed)
            ref.check_sample(z[~done], a[~done], w[~done], eps)
        seen = max(seen, int(done.sum()))
        env.step(torch.from_numpy(a).cuda())
    assert seen == 1 + len(range(0, B, 3)) - (1 if 5 % 3 == 0 else 0)   # the preset one and the finished ones
    assert _np(env.done).sum() == seen and seen < B


def test_sample_uses_the_global_env_id():
    """gid = env_id_offset + i: two handles of 32 envs with env_id_offset 0 and 32 draw what one handle of 64
    draws from the same obs and counters, and an offset above 2^32 reaches the counter's high word."""
    R, eps, seed = 2, 0.25, (9 << 32) | 4
    rng = np.random.default_rng(17)
    layers = ref.random_layers(rng, (14 * R, 7, 5, 10), scale=1.0)
    whole = _env(num_envs=64, action_repeats=R, seed=6)
    whole.reset()
    st = _np(whole.get_state())
    ints = abi.state_ints(st)
    ints[abi.CP_SF_STEPS] = rng.integers(0, 100, 64)
    ints[abi.CP_SF_EPISODE] = rng.integers(0, 1000, 64)
    steps, episode = ints[abi.CP_SF_STEPS].copy(), ints[abi.CP_SF_EPISODE].copy()
    whole.set_state(torch.from_numpy(st))
    whole.set_policy(_t(layers), "sample", epsilon=eps, seed=seed)
    obs = whole.obs.clone()
    z = ref.forward(layers, _np(obs).reshape(64, -1))
    a64 = _np(whole.policy_act())
    ref.check_sample(z, a64, ref.sample_words(steps, episode, np.arange(64), seed), eps)
    big = (1 << 32) + 7
    parts = {}
    for off in (0, 32, big):
        shard = _env(num_envs=32, action_repeats=R, seed=6, env_id_offset=off)
        shard.reset()
        lo = 32 if off == 32 else 0
        shard.set_state(torch.from_numpy(np.ascontiguousarray(st[:, lo:lo + 32])))
        shard.set_policy(_t(layers), "sample", epsilon=eps, seed=seed)
        parts[off] = _np(shard.policy_act(obs=obs[lo:lo + 32]))
    assert np.array_equal(np.concatenate([parts[0], parts[32]]), a64), "shards of 32 against one handle of 64"
    assert not np.array_equal(parts[0], a64[32:]) and not np.array_equal(parts[32], a64[:32])
    # the same logits and counters under another gid: other draws, the restatement's for that gid
    ref.check_sample(z[:32], parts[big], ref.sample_words(steps[:32], episode[:32], big + np.arange(32), seed), eps)
    assert not np.array_equal(parts[big], parts[0])
    w0 = ref.sample_words(steps[:32], episode[:32], 7 + np.arange(32), seed)   # the low word alone
    with pytest.raises(AssertionError):
        ref.check_sample(z[:32], parts[big], w0, eps)


def test_weights_are_read_live():
    from cartpoleplusplus_amd import policy
    B, R = 33, 2
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(12)
    l1, l2 = (ref.random_layers(rng, (14 * R, 7, 5, 10), scale=3.0) for _ in range(2))
    packed = env.set_policy(_t(l1), "argmax")
    x = _np(env.obs).reshape(B, -1)
    a1 = _np(env.policy_act())
    _assert_same(a1, ref.act_argmax(ref.forward(l1, x)), "first weights")
    ptr = packed.data_ptr()
    policy.repack(packed, _t(l2))        # an optimiser step: the same buffer, no set_policy
    assert packed.data_ptr() == ptr
    a2 = _np(env.policy_act())
    _assert_same(a2, ref.act_argmax(ref.forward(l2, x)), "overwritten weights")
    assert not np.array_equal(a1, a2)
    env.set_policy(None)


def _err(env):
    return env.lib.cp_last_error(env.h)


def test_rejections():
    rng = np.random.default_rng(0)
    R = 2
    layers = _t(ref.random_layers(rng, (14 * R, 6, 10)))
    from cartpoleplusplus_amd import policy
    packed, pol = policy.pack(layers, "argmax")
    lib = native.load()

    def rejected(env, needle, p=pol):
        assert lib.cp_set_policy(env.h, C.byref(p)) != 0
        assert needle in _err(env), _err(env)

    rejected(_env(num_envs=8, action_repeats=R, precision=abi.CP_PRECISION_F64), b"fp32 only")
    for flag in (abi.CP_MODEL_PERSISTENT, abi.CP_MODEL_SLEEPING):
        cfg = native.default_config(num_envs=8, action_repeats=R)
        cfg.phys.model_flags = flag
        rejected(BatchedCartpole(8, 0, config=cfg), b"CP_MODEL_PERSISTENT / CP_MODEL_SLEEPING")
    rejected(_env(num_envs=8, action_repeats=R, autoreset=abi.CP_AUTORESET_NEXT_STEP), b"CP_AUTORESET_NEXT_STEP")
    rejected(_env(num_envs=8, action_repeats=3), b"width[0] must be 14 * action_repeats = 42")
    env = _env(num_envs=8, action_repeats=R)
    from cartpoleplusplus_amd.lqr import exact_gains
    env.enable_lqr(torch.from_numpy(exact_gains()), state8=False)
    rejected(env, b"LQR policy on")
    env.enable_lqr(None)
    bad = abi.cp_policy.from_buffer_copy(pol)
    bad.head = abi.CP_HEAD_TANH
    rejected(env, b"out width must be 4", bad)
    bad = abi.cp_policy.from_buffer_copy(pol)
    bad.width[1] = 129
    rejected(env, b"width[1]", bad)
    bad = abi.cp_policy.from_buffer_copy(pol)
    bad.head, bad.epsilon = abi.CP_HEAD_SAMPLE, float("nan")
    rejected(env, b"epsilon", bad)
    # no policy yet: the calls that need one say so
    env.reset()
    a = torch.zeros((8, 2), dtype=torch.int8, device="cuda")
    assert lib.cp_policy_act(env.h, env.obs.data_ptr(), None, a.data_ptr(), None) != 0 and b"no policy" in _err(env)
    env.set_policy(layers, "argmax")
    # cp_set_lqr refuses a handle with a policy on
    with pytest.raises(native.CartpoleError, match="MLP policy on"):
        env.enable_lqr(torch.from_numpy(exact_gains()), state8=False)
    # shapes and dtypes through _device_buffer
    with pytest.raises(ValueError):
        env.policy_act(obs=torch.zeros((8, 3, 2, 7), device="cuda"))
    with pytest.raises(ValueError):
        env.policy_act(noise=torch.zeros((8, 2), device="cuda"))
    a = env.policy_act()
    assert a.shape == (8, 2) and a.dtype == torch.int8


@pytest.mark.parametrize("autoreset", [0, 1])
def test_step_and_rollout_unchanged_with_a_policy_set(autoreset):
    """cp_step and cp_rollout ignore a policy: the same bits with and without one."""
    B, R, K = 64, 2, 12
    rng = np.random.default_rng(3)
    layers = _t(ref.random_layers(rng, (14 * R, 6, 10)))
    acts = torch.from_numpy(rng.integers(0, 5, (K, B, 2)).astype(np.int8)).cuda()
    outs = []
    for with_policy in (False, True):
        env = _env(num_envs=B, action_repeats=R, seed=2, autoreset=autoreset, max_episode_len=5)
        if with_policy:
            env.set_policy(layers, "argmax")
        env.reset()
        steps = [tuple(x.clone() for x in env.step(acts[k])) for k in range(4)]
        roll = tuple(x.clone() for x in env.rollout(acts[4:]))
        outs.append((steps, roll, env.get_state()))
    for k in range(4):
        for x, y in zip(outs[0][0][k], outs[1][0][k]):
            _same(x, y, f"step {k}")
    for x, y in zip(outs[0][1], outs[1][1]):
        _same(x, y, "rollout")
    _same(outs[0][2], outs[1][2], "state")
