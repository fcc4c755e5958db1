"""In-kernel exploration noise of cp_policy_act on the MI355X (cp_set_policy_noise): the Gaussian draws against
the float64 restatement (tests/policy_noise_ref.py), the head and the OU update bit for bit given those draws,
the clips, done envs, sharding, both population kernels, noise off = the call as it was, and the rejections.
CLIP head with widths (14 R, 7, 4) and R = 2 unless a case says otherwise."""
import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native
from tests import policy_noise_ref as nref
from tests import policy_ref as ref
from tests.test_gpu_parity import _assert_same, _np
from tests.test_gpu_policy import _env, _same, _t
from tests.test_gpu_policy_population import _members, _z

pytestmark = pytest.mark.gpu

R = 2
SIGMA = 0.3
# the largest |n_dev - n64| / (sigma * max(1, r)) over test_gaussian_and_the_head's draws, measured on the MI355X
# (2.4 x 2^-24; B = 3: 1.313e-07).  The bound is 4 x that (logf, sqrtf, sinf and cosf errors compose), and never
# above policy_ref.DELTA = 2^-18
GAUSS_MEASURED = 1.406e-07
GAUSS_BOUND = min(4 * GAUSS_MEASURED, nref.DELTA)


def _fresh(B, **kw):
    kw.setdefault("seed", 11)
    env = _env(num_envs=B, action_repeats=R, **kw)
    env.reset()
    return env


def _counters(env):
    ints = abi.state_ints(_np(env.get_state()))
    return ints[abi.CP_SF_STEPS].copy(), ints[abi.CP_SF_EPISODE].copy(), ints[abi.CP_SF_DONE].copy()


def _gauss_err(n_dev, words, sigma=SIGMA):
    """max |n_dev - sigma * g64| / (sigma * max(1, r)) over the rows of n_dev (B, 4)."""
    g, r = nref.gauss64(words)
    s = float(np.float32(sigma))
    return float((np.abs(n_dev.astype(np.float64) - s * g) / (s * np.maximum(1.0, r))).max())


@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("net", ["small", "wide", "tanh"])
def test_gaussian_and_the_head(net, B):
    """Six steps over two episodes (max_episode_len = 3, autoreset); B = 130: env 129 sits in a partial wave.
    Every draw of every step is compared, and the action is exact given the noise the kernel reports."""
    seed = (7 << 32) | 21
    env = _fresh(B, autoreset=1, max_episode_len=3)
    rng = np.random.default_rng(B)
    widths = (14 * R, 100, 100, 50, 4) if net == "wide" else (14 * R, 7, 4)
    layers = ref.random_layers(rng, widths, scale=6.0 if net == "tanh" else 1.5)
    env.set_policy(_t(layers), "tanh" if net == "tanh" else "clip")
    env.set_policy_noise("gaussian", sigma=SIGMA, max_magnitude=0.0, seed=seed)
    worst, seen = 0.0, set()
    for k in range(6):
        steps, episode, done = _counters(env)
        assert not done.any()
        seen.update(zip(steps.tolist(), episode.tolist()))
        z = ref.forward(layers, _np(env.obs).reshape(B, -1))
        a = env.policy_act()
        n = _np(env.policy_noise)
        err = _gauss_err(n.reshape(B, 4), nref.noise_words(steps, episode, np.arange(B), seed))
        worst = max(worst, err)
        if net == "tanh":
            exp = np.clip(np.tanh(z.astype(np.float64)) + n.reshape(B, 4), -1.0, 1.0)
            assert np.abs(_np(a).reshape(B, 4) - exp).max() <= 1e-6
        else:
            _assert_same(_np(a), ref.act_clip(z, n), f"step {k}: the head given the noise")
        env.step(a)
    print(f"gaussian {net} B={B}: max |n_dev - n64| / (sigma max(1, r)) = {worst:.3e} (bound {GAUSS_BOUND:.3e})")
    assert len({e for _, e in seen}) >= 2 and {s for s, _ in seen} == {0, 1, 2}
    assert worst <= GAUSS_BOUND


@pytest.mark.parametrize("reset_on_episode", [False, True])
def test_ou_is_exact_given_the_gaussian_stream(reset_on_episode):
    """Two handles, one GAUSSIAN(sigma), one OU(theta, sigma), the same config, seeds and actions: the OU state
    after a step is ou_update(its state before, the Gaussian handle's n bits), raw bits, for 8 steps over
    episode ends (max_episode_len = 3)."""
    B, theta, seed = 67, 0.15, 99
    flags = nref.RESET_ON_EPISODE if reset_on_episode else 0
    rng = np.random.default_rng(2)
    layers = _t(ref.random_layers(rng, (14 * R, 7, 4)))
    act = torch.from_numpy(rng.uniform(-1, 1, (B, 2, 2)).astype(np.float32)).cuda()
    gh, oh = (_fresh(B, autoreset=1, max_episode_len=3) for _ in range(2))
    for env in (gh, oh):
        env.set_policy(layers, "clip")
    gh.set_policy_noise("gaussian", sigma=SIGMA, max_magnitude=0.0, seed=seed)
    oh.set_policy_noise("ou", theta=theta, sigma=SIGMA, max_magnitude=0.0, seed=seed, reset_on_episode=reset_on_episode)
    restarts = 0
    for k in range(8):
        steps, episode, _ = _counters(oh)
        gs, ge, _ = _counters(gh)
        assert np.array_equal(steps, gs) and np.array_equal(episode, ge)
        before = _np(oh.policy_noise).reshape(B, 4)
        gh.policy_act()
        oh.policy_act()
        n = _np(gh.policy_noise).reshape(B, 4)
        after = _np(oh.policy_noise).reshape(B, 4)
        _assert_same(after, nref.ou_update(before, n, theta, flags, 0.0, steps), f"step {k}")
        if k > 0 and (steps == 0).all():      # the first step of a later episode
            restarts += 1
            assert np.abs(before).min() > 0
            if reset_on_episode:
                _assert_same(after, n, "x = 0 before the update: the state is the draw")
            else:
                assert not np.array_equal(after, n), "the state is carried over the reset"
        gh.step(act)
        oh.step(act)
    assert restarts == 2


@pytest.mark.parametrize("mode", ["default", "symmetric", "none"])
def test_clip_without_libm(mode):
    """theta = 0 and sigma = 0: the update adds zeros, so the state set through the setter meets the clip alone."""
    B, m = 6, 1.5
    env = _fresh(B)
    rng = np.random.default_rng(3)
    layers = ref.random_layers(rng, (14 * R, 7, 4), scale=0.05)
    env.set_policy(_t(layers), "clip")
    env.set_policy_noise("ou", theta=0.0, sigma=0.0, max_magnitude=0.0 if mode == "none" else m,
                         symmetric_clip=mode == "symmetric")
    x = np.array([[m + 1, -(m + 1), m / 2, -m / 2]] * B, np.float32)
    x[1] = [m, -m, np.nextafter(np.float32(m), np.float32(2)), -np.nextafter(np.float32(m), np.float32(2))]
    x[2] *= -1
    env.policy_noise = torch.from_numpy(x.reshape(B, 2, 2))
    _assert_same(_np(env.policy_noise), x.reshape(B, 2, 2), "the setter")
    a = env.policy_act()
    got = _np(env.policy_noise).reshape(B, 4)
    exp = {"default": np.minimum(x, np.float32(m)), "symmetric": np.clip(x, np.float32(-m), np.float32(m)), "none": x}[mode]
    _assert_same(got, exp, mode)
    assert got[0, 0] == (m + 1 if mode == "none" else m) and got[0, 1] == (-m if mode == "symmetric" else -(m + 1))
    _assert_same(_np(a), ref.act_clip(ref.forward(layers, _np(env.obs).reshape(B, -1)), got), "the head uses the clipped x")


def test_done_envs_keep_their_state_rows():
    B, seed = 33, 5
    env = _fresh(B, autoreset=0, max_episode_len=2)
    st = _np(env.get_state())
    done = np.zeros(B, bool)
    done[[0, 5, 17, B - 1]] = True
    abi.state_ints(st)[abi.CP_SF_DONE][done] = 1
    env.set_state(torch.from_numpy(st))
    rng = np.random.default_rng(21)
    layers = ref.random_layers(rng, (14 * R, 7, 4), scale=0.05)
    env.set_policy(_t(layers), "clip")
    env.set_policy_noise("ou", theta=0.15, sigma=SIGMA, seed=seed)
    x0 = rng.uniform(0.3, 0.5, (B, 2, 2)).astype(np.float32)
    env.policy_noise = torch.from_numpy(x0)
    a = _np(env.policy_act())
    x1 = _np(env.policy_noise)
    assert not a[done].any(), "a done env's action is 0"
    _assert_same(x1[done], x0[done], "done envs: rows untouched")
    assert (x1[~done].reshape(-1, 4) != x0[~done].reshape(-1, 4)).all(), "live envs advance"
    _assert_same(a[~done], ref.act_clip(ref.forward(layers, _np(env.obs).reshape(B, -1)), x1)[~done], "live envs")
    for _ in range(2):                       # past the episode length: every env is done now
        env.step(env.policy_act())
    assert _counters(env)[2].all()
    x2 = _np(env.policy_noise)
    assert not _np(env.policy_act()).any()
    _assert_same(_np(env.policy_noise), x2, "all done: no row moves")
    _assert_same(x2[done], x0[done], "never evaluated")


def test_sharding_and_the_high_word():
    """gid = env_id_offset + i: two handles of 32 envs at env_id_offset 0 and 32 draw, bit for bit, what one
    handle of 64 draws from the same obs and counters (OU: two calls, the state carried); an offset above 2^32
    changes the draws to the restatement's for that gid."""
    seed = (9 << 32) | 4
    rng = np.random.default_rng(17)
    layers = _t(ref.random_layers(rng, (14 * R, 7, 4)))
    whole = _fresh(64, seed=6)
    st = _np(whole.get_state())
    ints = abi.state_ints(st)
    ints[abi.CP_SF_STEPS] = rng.integers(0, 100, 64)
    ints[abi.CP_SF_EPISODE] = rng.integers(0, 1000, 64)
    steps, episode = ints[abi.CP_SF_STEPS].copy(), ints[abi.CP_SF_EPISODE].copy()
    whole.set_state(torch.from_numpy(st))
    whole.set_policy(layers, "clip")
    obs = whole.obs.clone()
    big = (1 << 32) + 7
    shards = {}
    for off in (0, 32, big):
        shard = _fresh(32, seed=6, env_id_offset=off)
        lo = 32 if off == 32 else 0
        shard.set_state(torch.from_numpy(np.ascontiguousarray(st[:, lo:lo + 32])))
        shard.set_policy(layers, "clip")
        shards[off] = (shard, obs[lo:lo + 32].contiguous())
    for kind in ("gaussian", "ou"):
        def run(env, o):
            env.set_policy_noise(kind, theta=0.15, sigma=SIGMA, max_magnitude=0.0, seed=seed)
            env.policy_noise = None
            out = []
            for _ in range(2):
                out += [_np(env.policy_act(obs=o)).copy(), _np(env.policy_noise).copy()]
            return out
        w = run(whole, obs)
        p = {off: run(*shards[off]) for off in shards}
        for k in range(4):
            _assert_same(np.concatenate([p[0][k], p[32][k]]), w[k], f"{kind}: shards of 32 against one handle of 64")
        assert not np.array_equal(p[0][1], w[1][32:]) and not np.array_equal(p[big][1], p[0][1])
        if kind == "gaussian":
            n_big = p[big][1].reshape(32, 4)
            assert _gauss_err(n_big, nref.noise_words(steps[:32], episode[:32], big + np.arange(32), seed)) <= GAUSS_BOUND
            assert _gauss_err(n_big, nref.noise_words(steps[:32], episode[:32], 7 + np.arange(32), seed)) > 0.01  # low word alone
            assert _gauss_err(w[1].reshape(64, 4), nref.noise_words(steps, episode, np.arange(64), seed)) <= GAUSS_BOUND


def test_both_population_kernels():
    """Wave-uniform path (G = 64, P = 3, B = 200) and member path (G = 5, P = 3, B = 33): the actions are
    act_clip(z of the env's member, policy_noise) exactly, and for equal gid, steps and episode the two paths'
    Gaussian n are the same bits."""
    P, seed = 3, 1234
    rng = np.random.default_rng(8)
    raw = _members(rng, (14 * R, 7, 4), P)
    ns, counters = {}, set()
    for G, B in ((64, 200), (5, 33)):
        env = _fresh(B)
        env.set_policy([_t(m) for m in raw], "clip", group=G)
        z, mem = _z(raw, _np(env.obs).reshape(B, -1), G)
        assert len(np.unique(mem)) == P
        steps, episode, _ = _counters(env)
        for kind in ("ou", "gaussian"):
            env.set_policy_noise(kind, theta=0.15, sigma=SIGMA, max_magnitude=0.0, seed=seed)
            for _ in range(2):
                a = _np(env.policy_act())
                n = _np(env.policy_noise)
                _assert_same(a, ref.act_clip(z, n), f"G = {G}, {kind}")
        ns[G] = n
        assert _gauss_err(n.reshape(B, 4), nref.noise_words(steps, episode, np.arange(B), seed)) <= GAUSS_BOUND
        assert not steps.any() and len(set(episode.tolist())) == 1      # the same counters on both handles
        counters.add(int(episode[0]))
    assert len(counters) == 1
    _assert_same(ns[5], ns[64][:33], "the member path's n against the wave-uniform path's")


def test_off_is_the_call_as_it_was():
    B = 70
    rng = np.random.default_rng(12)
    layers = _t(ref.random_layers(rng, (14 * R, 7, 4)))
    noise = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 2, 2)).astype(np.float32)).cuda()
    plain, used = _fresh(B), _fresh(B)
    for env in (plain, used):
        env.set_policy(layers, "tanh")
    used.set_policy_noise("ou", theta=0.15, sigma=SIGMA, seed=3)
    a_noisy = used.policy_act().clone()
    used.policy_act()
    x = used.policy_noise.clone()
    used.set_policy_noise(None)
    _same(used.policy_act(), plain.policy_act(), "policy_act() after noise off")
    _same(used.policy_act(noise=noise), plain.policy_act(noise=noise), "policy_act(noise=...) after noise off")
    assert not np.array_equal(_np(a_noisy), _np(plain.policy_act()))
    _same(used.policy_noise, x, "off keeps the state")
    used.set_policy_noise("off")
    used.set_policy_noise("ou", theta=0.15, sigma=SIGMA, seed=3)
    _same(used.policy_noise, x, "the state survives an off / on cycle")
    assert _np(x).any()
    used.policy_noise = None
    assert not _np(used.policy_noise).any()


@pytest.mark.parametrize("autoreset", [0, 1])
def test_step_and_rollout_unchanged_with_noise_set(autoreset):
    B, K = 64, 12
    rng = np.random.default_rng(3)
    layers = _t(ref.random_layers(rng, (14 * R, 6, 4)))
    acts = torch.from_numpy(rng.uniform(-1, 1, (K, B, 2, 2)).astype(np.float32)).cuda()
    outs = []
    for with_noise in (False, True):
        env = _env(num_envs=B, action_repeats=R, seed=2, autoreset=autoreset, max_episode_len=5)
        if with_noise:
            env.set_policy(layers, "clip")
            env.set_policy_noise("ou", theta=0.15, sigma=SIGMA, seed=1)
        env.reset()
        steps = [tuple(x.clone() for x in env.step(acts[k])) for k in range(4)]
        if with_noise:
            env.policy_act()
        roll = tuple(x.clone() for x in env.rollout(acts[4:]))
        outs.append((steps, roll, env.get_state()))
    for k in range(4):
        for x, y in zip(outs[0][0][k], outs[1][0][k]):
            _same(x, y, f"step {k}")
    for x, y in zip(outs[0][1], outs[1][1]):
        _same(x, y, "rollout")
    _same(outs[0][2], outs[1][2], "state")


def test_rejections():
    B = 8
    rng = np.random.default_rng(0)
    env = _fresh(B)
    # before any noise has been set there is no state to get or set
    with pytest.raises(native.CartpoleError, match="no noise has been set"):
        env.policy_noise
    with pytest.raises(native.CartpoleError, match="no noise has been set"):
        env.policy_noise = torch.zeros((B, 2, 2), device="cuda")
    with pytest.raises(native.CartpoleError, match="no noise has been set"):
        env.policy_noise = None
    # whatever cp_policy_noise_check rejects, and an unknown name
    with pytest.raises(native.CartpoleError, match="sigma must be finite"):
        env.set_policy_noise("ou", sigma=-1.0)
    with pytest.raises(native.CartpoleError, match="theta must be finite"):
        env.set_policy_noise("ou", theta=float("nan"))
    with pytest.raises(ValueError, match="kind must be one of"):
        env.set_policy_noise("brownian")
    with pytest.raises(native.CartpoleError, match="no noise has been set"):   # the rejected calls allocated nothing
        env.policy_noise
    # a discrete head with noise on, at cp_policy_act
    env.set_policy(_t(ref.random_layers(rng, (14 * R, 6, 10))), "argmax")
    env.set_policy_noise("gaussian", sigma=SIGMA)
    with pytest.raises(native.CartpoleError, match="discrete head"):
        env.policy_act()
    env.set_policy_noise(None)
    assert env.policy_act().shape == (B, 2)
    # a caller noise together with in-kernel noise
    env.set_policy(_t(ref.random_layers(rng, (14 * R, 6, 4))), "clip")
    env.set_policy_noise("gaussian", sigma=SIGMA)
    with pytest.raises(native.CartpoleError, match="caller noise pointer together with in-kernel noise"):
        env.policy_act(noise=torch.zeros((B, 2, 2), device="cuda"))
    assert env.policy_act().shape == (B, 2, 2)
    # a wrong shape or dtype through the setter
    with pytest.raises(ValueError):
        env.policy_noise = torch.zeros((B, 4), device="cuda")
    with pytest.raises(ValueError):
        env.policy_noise = torch.zeros((B + 1, 2, 2), device="cuda")
    with pytest.raises(ValueError):
        env.policy_noise = torch.zeros((B, 2, 2), dtype=torch.int32, device="cuda")
    # an fp64 handle
    env64 = _env(num_envs=B, action_repeats=R, precision=abi.CP_PRECISION_F64)
    with pytest.raises(native.CartpoleError, match="fp32 only"):
        env64.set_policy_noise("ou")
