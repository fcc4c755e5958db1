"""Seeded ES perturbations on the MI355X (cp_set_policy_es): cp_policy_act forming member m's weights
theta + s sigma eps while it stages them, cp_policy_es_weights and cp_policy_es_gradient.  The expected values
are tests/policy_es_ref.py's weights fed to tests/policy_ref.py's `forward` and heads, once per member; bit for bit
wherever the contract fixes every rounding.  The nets are the smallest at which staging can go wrong: F = 169
(Philox blocks straddle every layer boundary, the last block is partial), the four-layer net, and a 128-wide
layer (two units per lane, the raised LDS limit)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, policy
from tests import policy_es_ref as eref
from tests import policy_ref as ref
from tests.test_gpu_parity import _assert_same, _np
from tests.test_gpu_policy import _env, _obs_after_reset, _same, _t

pytestmark = pytest.mark.gpu

SIGMA, SEED, GEN = 0.11, (5 << 32) | 77, 3
NETS = {"R1": (14, 7, 5), "wide": (42, 100, 100, 50), "w128": (42, 128)}


def _widths(ws, head):
    return NETS[ws] + (4 if head in ("clip", "tanh") else 10,)


def _R(ws):
    return NETS[ws][0] // 14


def _flags(anti):
    return eref.ANTITHETIC if anti else 0


def _es_on(env, P, G, anti=True, sigma=SIGMA, seed=SEED, generation=GEN):
    env.set_policy_es(P, sigma, group=G, seed=seed, generation=generation, antithetic=anti)


def _z(theta, widths, x, P, G, anti, off=0, sigma=SIGMA, seed=SEED, generation=GEN):
    """The last layer's outputs per env: forward once per member, on that member's rows, with es_weights' row."""
    mem = policy.member_of(off + np.arange(x.shape[0], dtype=np.int64), G, P)
    used = np.unique(mem)
    W = eref.es_weights(theta, used, sigma, seed, generation, _flags(anti))
    z = np.zeros((x.shape[0], widths[-1]), np.float32)
    for k, m in enumerate(used):
        z[mem == m] = ref.forward(eref.unpacked(W[k], widths), x[mem == m])
    return z, mem


@pytest.fixture
def es_off():
    """The handles of _obs_after_reset are shared with the other policy tests: leave them with ES and policy off."""
    used = []
    yield used.append
    for env in used:
        env.set_policy_es(None)
        env.set_policy_noise(None)
        env.set_policy(None)


# ---- cp_policy_es_weights

@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
@pytest.mark.parametrize("P", [1, 2, 7, 3, 33, 130])
@pytest.mark.parametrize("ws", ["R1", "wide", "w128"])
def test_es_weights_bit_exact(ws, P, anti, es_off):
    """All members, and a sub-range with member_lo > 0; odd P with ANTITHETIC leaves the last pair one member."""
    env = _obs_after_reset(3, _R(ws))
    es_off(env)
    widths = _widths(ws, "clip")
    rng = np.random.default_rng(P)
    packed = env.set_policy(_t(ref.random_layers(rng, widths, scale=1.5)), "clip")
    theta = _np(packed)
    _es_on(env, P, 1, anti)
    want = eref.es_weights(theta, np.arange(P), SIGMA, SEED, GEN, _flags(anti))
    got = _np(env.policy_es_weights())
    assert got.shape == (P, theta.size)
    _assert_same(got, want, "all members")
    assert P == 1 or len(np.unique(got, axis=0)) == P
    if P > 2:
        lo, n = P // 2, P - P // 2 - 1
        _assert_same(_np(env.policy_es_weights(lo, n)), want[lo:lo + n], "members lo .. lo + n - 1")


@pytest.mark.parametrize("ws", ["R1", "wide"])
def test_centre_at_a_4_byte_offset(ws, es_off):
    """The centre one float into a 16-byte aligned buffer: the weights and the actions are those of the aligned one."""
    B, P, G = 33, 7, 2
    env = _obs_after_reset(B, _R(ws))
    es_off(env)
    widths = _widths(ws, "clip")
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(1), widths, scale=1.5)), "clip")
    _es_on(env, P, G)
    w0, a0 = env.policy_es_weights().clone(), env.policy_act().clone()
    buf = torch.zeros(packed.numel() + 1, device=packed.device)
    buf[1:] = packed
    assert buf.data_ptr() % 16 == 0
    pol = abi.cp_policy.from_buffer_copy(env.policy)
    pol.weights = buf.data_ptr() + 4
    native.check(env.h, env.lib.cp_set_policy(env.h, C.byref(pol)), "cp_set_policy")
    _same(env.policy_es_weights(), w0, "weights from the offset centre")
    _same(env.policy_act(), a0, "actions from the offset centre")
    _assert_same(_np(w0), eref.es_weights(_np(packed), np.arange(P), SIGMA, SEED, GEN), "against the restatement")


# ---- cp_policy_act with ES on

_POP = {}


def _population_handle(B, R):
    """A second handle per (B, R) for the materialised [P][F] population (any reset state: the obs are passed in)."""
    if (B, R) not in _POP:
        _POP[(B, R)] = _env(num_envs=B, action_repeats=R, seed=11)
        _POP[(B, R)].reset()
    return _POP[(B, R)]


def _population_act(pop, env, W, G, obs, noise):
    """policy_act of the shipped population kernels on the rows W [P][F] (cp_policy_es_weights' output)."""
    pol = abi.cp_policy.from_buffer_copy(env.policy)
    pol.weights, pol.population, pol.group = W.data_ptr(), W.shape[0], G
    native.check(pop.h, pop.lib.cp_set_policy(pop.h, C.byref(pol)), "cp_set_policy")
    pop.policy, pop.policy_weights = pol, W
    try:
        return pop.policy_act(obs=obs, noise=noise).clone()
    finally:
        pop.set_policy(None)


@pytest.mark.parametrize("B", [3, 33, 130])
@pytest.mark.parametrize("P", [1, 2, 7, "B"])
@pytest.mark.parametrize("G", [1, 2, 5, 64, 96])
@pytest.mark.parametrize("ws", ["R1", "wide", "w128"])
def test_es_act_bit_exact(ws, G, P, B, es_off):
    """CLIP + caller noise and ARGMAX against the restatement and against the materialised population on a second
    handle.  G = 64 and 96 are the groups the population kernels would serve one member per wave."""
    P = B if P == "B" else P
    anti = (G + P) % 3 != 0          # both settings over the grid, ANTITHETIC the more frequent one
    env = _obs_after_reset(B, _R(ws))
    es_off(env)
    pop = _population_handle(B, _R(ws))
    x = _np(env.obs).reshape(B, -1)
    for head in ("clip", "argmax"):
        widths = _widths(ws, head)
        rng = np.random.default_rng(1000 * G + 10 * P + B + (head == "clip"))
        packed = env.set_policy(_t(ref.random_layers(rng, widths, scale=1.5)), head)
        _es_on(env, P, G, anti)
        z, _ = _z(_np(packed), widths, x, P, G, anti)
        noise = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 2, 2)).astype(np.float32)) if head == "clip" else None
        a = env.policy_act(noise=noise)
        if head == "clip":
            _assert_same(_np(a), ref.act_clip(z, noise.numpy()), "clip + noise")
        else:
            _assert_same(_np(a), ref.act_argmax(z), "argmax")
        _same(_population_act(pop, env, env.policy_es_weights(), G, env.obs, noise), a, f"{head}: the population kernels")
        env.set_policy_es(None)


@pytest.mark.parametrize("G,B", [(1, 33), (5, 33), (96, 130)])
def test_tanh_with_es(G, B, es_off):
    """|a - float32(tanh64(z))| <= 1e-6: test_policy_act_tanh's bound (z is exact in the restatement)."""
    R, P, widths = 3, 7, (42, 7, 5, 4)
    env = _obs_after_reset(B, R)
    es_off(env)
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(G), widths, scale=6.0)), "tanh")
    _es_on(env, P, G, sigma=0.5)
    z, _ = _z(_np(packed), widths, _np(env.obs).reshape(B, -1), P, G, True, sigma=0.5)
    a = _np(env.policy_act()).reshape(B, 4)
    err = np.abs(a.astype(np.float64) - np.tanh(z.astype(np.float64)).astype(np.float32).astype(np.float64)).max()
    print(f"tanh head with ES: max |a - tanh64(z)| = {err:.3g}, |z| up to {np.abs(z).max():.3g}")
    assert err <= 1e-6
    assert np.abs(z).max() > 0.5 and np.abs(a).max() <= 1.0


def test_sample_with_es_and_shards():
    """As test_sample_population: G = 8, P = 5, B = 64, the epsilon draws exact, the others inside check_sample's
    interval; two handles of 32 envs at offsets 0 and 32 draw what the handle of 64 draws."""
    B, R, G, P, eps, seed = 64, 2, 8, 5, 0.25, (9 << 32) | 4
    widths = (14 * R, 7, 5, 10)
    rng = np.random.default_rng(31)
    layers = _t(ref.random_layers(rng, widths, scale=1.0))
    whole = _env(num_envs=B, action_repeats=R, seed=6)
    whole.reset()
    st = _np(whole.get_state())
    ints = abi.state_ints(st)
    ints[abi.CP_SF_STEPS] = rng.integers(0, 100, B)
    ints[abi.CP_SF_EPISODE] = rng.integers(0, 1000, B)
    steps, episode = ints[abi.CP_SF_STEPS].copy(), ints[abi.CP_SF_EPISODE].copy()
    whole.set_state(torch.from_numpy(st))
    packed = whole.set_policy(layers, "sample", epsilon=eps, seed=seed)
    _es_on(whole, P, G, sigma=0.3)
    obs = whole.obs.clone()
    z, mem = _z(_np(packed), widths, _np(obs).reshape(B, -1), P, G, True, sigma=0.3)
    assert len(np.unique(mem)) == P and mem[40] == 0          # the members wrap inside the batch
    a64 = _np(whole.policy_act())
    n_eps, n_soft, near = ref.check_sample(z, a64, ref.sample_words(steps, episode, np.arange(B), seed), eps)
    assert n_eps > 0 and n_soft > n_eps and near < 0.05
    parts = []
    for off in (0, 32):
        shard = _env(num_envs=32, action_repeats=R, seed=6, env_id_offset=off)
        shard.reset()
        shard.set_state(torch.from_numpy(np.ascontiguousarray(st[:, off:off + 32])))
        shard.set_policy(layers, "sample", epsilon=eps, seed=seed)
        _es_on(shard, P, G, sigma=0.3)
        parts.append(_np(shard.policy_act(obs=obs[off:off + 32].contiguous())))
    assert np.array_equal(np.concatenate(parts), a64), "shards of 32 against one handle of 64"


@pytest.mark.parametrize("G,P", [(1, 64), (5, 7), (96, 3)])
def test_shards_equal_the_whole(G, P):
    """CLIP: two handles of 32 envs at offsets 0 and 32 give the actions of one handle of 64, raw bits."""
    R, widths = 3, (42, 7, 5, 4)
    layers = _t(ref.random_layers(np.random.default_rng(G), widths, scale=1.5))
    whole = _obs_after_reset(64, R)
    obs = whole.obs.clone()
    try:
        whole.set_policy(layers, "clip")
        _es_on(whole, P, G)
        a = whole.policy_act().clone()
    finally:
        whole.set_policy_es(None)
        whole.set_policy(None)
    for off in (0, 32):
        shard = _env(num_envs=32, action_repeats=R, seed=11, env_id_offset=off)
        shard.reset()
        shard.set_policy(layers, "clip")
        _es_on(shard, P, G)
        _same(shard.policy_act(obs=obs[off:off + 32].contiguous()), a[off:off + 32], f"shard at {off}")
    assert len(np.unique(_np(a).reshape(64, -1), axis=0)) > 1


def test_offset_above_2_to_the_32():
    """env_id_offset = 2^32 + 5 with G = 2, P = 7: the member comes from 64-bit arithmetic (2^31 mod 7 = 2, so the
    low 32 bits of the global id alone give other members)."""
    B, R, G, P, widths, off = 33, 3, 2, 7, (42, 7, 5, 4), (1 << 32) + 5
    env = _env(num_envs=B, action_repeats=R, seed=11, env_id_offset=off)
    env.reset()
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(4), widths, scale=1.5)), "clip")
    _es_on(env, P, G)
    z, mem = _z(_np(packed), widths, _np(env.obs).reshape(B, -1), P, G, True, off=off)
    assert (mem != policy.member_of(5 + np.arange(B), G, P)).all()
    _assert_same(_np(env.policy_act()), ref.act_clip(z), "offset above 2^32")


@pytest.mark.parametrize("G,B", [(1, 33), (5, 33), (96, 130)])
def test_done_envs_get_zero_actions(G, B):
    """Done envs get 0, the others the restatement: single envs of a run, one of an antithetic pair (G = 1: env 1
    of the pair 0, 1), and a whole chunk (G = 1, 5: envs 20 .. 24; G = 96: the run's first 64 envs)."""
    R, P, widths = 2, 6, (28, 7, 5, 4)
    env = _env(num_envs=B, action_repeats=R, seed=3, autoreset=0)
    env.reset()
    st = _np(env.get_state())
    done = np.zeros(B, bool)
    done[[1, 7, 12, B - 1]] = True
    done[20:25] = True
    if G == 96:
        done[0:64] = True
    abi.state_ints(st)[abi.CP_SF_DONE][done] = 1
    env.set_state(torch.from_numpy(st))
    rng = np.random.default_rng(21)
    packed = env.set_policy(_t(ref.random_layers(rng, widths, scale=2.0)), "clip")
    _es_on(env, P, G)
    z, _ = _z(_np(packed), widths, _np(env.obs).reshape(B, -1), P, G, True)
    noise = rng.uniform(0.3, 0.5, (B, 2, 2)).astype(np.float32)
    a = _np(env.policy_act(noise=torch.from_numpy(noise)))
    assert not a[done].any(), "a done env's action is 0"
    _assert_same(a[~done], ref.act_clip(z, noise)[~done], "live envs")
    assert np.abs(a[~done]).min() > 0


def test_live_centre_and_generation(es_off):
    """theta overwritten in place: the next launch follows.  Another generation gives other actions."""
    B, R, P, G, widths = 33, 2, 7, 2, (28, 7, 5, 4)
    env = _obs_after_reset(B, R)
    es_off(env)
    rng = np.random.default_rng(12)
    packed = env.set_policy(_t(ref.random_layers(rng, widths, scale=0.05)), "clip")   # small: nothing saturates
    x = _np(env.obs).reshape(B, -1)
    _es_on(env, P, G, sigma=0.02)
    a1 = _np(env.policy_act()).copy()
    _assert_same(a1, ref.act_clip(_z(_np(packed), widths, x, P, G, True, sigma=0.02)[0]), "first centre")
    ptr = packed.data_ptr()
    policy.repack(packed, _t(ref.random_layers(rng, widths, scale=0.05)))
    assert packed.data_ptr() == ptr
    a2 = _np(env.policy_act()).copy()
    _assert_same(a2, ref.act_clip(_z(_np(packed), widths, x, P, G, True, sigma=0.02)[0]), "overwritten centre")
    assert (a2.reshape(B, -1) != a1.reshape(B, -1)).any(axis=1).all()
    _es_on(env, P, G, sigma=0.02, generation=GEN + 1)
    a3 = _np(env.policy_act())
    _assert_same(a3, ref.act_clip(_z(_np(packed), widths, x, P, G, True, sigma=0.02, generation=GEN + 1)[0]), "generation")
    assert (a3.reshape(B, -1) != a2.reshape(B, -1)).any(axis=1).all()


def test_es_with_in_kernel_ou_noise(es_off):
    """The exploration noise does not depend on the member: the n reported with ES on is the ES-off run's n, and the
    action is clip(z' + n) on the perturbed z'."""
    B, R, P, G, widths = 33, 3, 7, 2, (42, 7, 5, 4)
    env = _obs_after_reset(B, R)
    es_off(env)
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(2), widths, scale=0.3)), "clip")
    env.set_policy_noise("ou", theta=0.15, sigma=0.2, seed=99)
    x = _np(env.obs).reshape(B, -1)
    env.policy_noise = None
    a_off, n_off = _np(env.policy_act()).copy(), _np(env.policy_noise).copy()
    _es_on(env, P, G)
    env.policy_noise = None
    a_on, n_on = _np(env.policy_act()).copy(), _np(env.policy_noise).copy()
    _assert_same(n_on, n_off, "the noise with ES on")
    assert n_on.any()
    _assert_same(a_on, ref.act_clip(_z(_np(packed), widths, x, P, G, True)[0], n_on), "clip(z' + n)")
    _assert_same(a_off, ref.act_clip(ref.forward(eref.unpacked(_np(packed), widths), x), n_off), "ES off")


# ---- cp_policy_es_gradient

@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
@pytest.mark.parametrize("P", [1, 7, 130])
@pytest.mark.parametrize("ws", ["R1", "wide"])
def test_es_gradient(ws, P, anti, es_off):
    """Per parameter |g - g64| <= gamma_(n+2) * sum_m |coeff_m eps_m|, n the members summed: every term is a
    product (one rounding; with ANTITHETIC one more for c_2k - c_2k+1) and any summation order of n terms adds at
    most n - 1 roundings, so the bound holds for any order (Higham, Accuracy and Stability, section 4.2).  Ranges,
    random and all-equal coeff; two calls give identical bits."""
    env = _obs_after_reset(3, _R(ws))
    es_off(env)
    widths = _widths(ws, "clip")
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(0), widths)), "clip")
    F = packed.numel()
    _es_on(env, P, 1, anti)
    rng = np.random.default_rng(P)
    for lo, n in sorted({(0, P), (P // 2, P - P // 2), (P // 3, max(P // 3, 1)), (P - 1, 1)}):
        for coeff in (rng.standard_normal(n).astype(np.float32), np.full(n, 0.75, np.float32)):
            first = env.policy_es_gradient(torch.from_numpy(coeff), lo)
            g = _np(first)
            g64, scale = eref.es_gradient64(coeff, lo, F, SEED, GEN, _flags(anti))
            assert g.shape == (F,) and g.dtype == np.float32
            err, bound = np.abs(g.astype(np.float64) - g64), eref.gamma(n + 2) * scale
            print(f"{ws} P={P} lo={lo} n={n}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
            assert (err <= bound).all()
            assert g.any() or (anti and n > 1 and coeff[0] == coeff[-1])
            _same(env.policy_es_gradient(torch.from_numpy(coeff), lo), first, "a second call")


@pytest.mark.parametrize("P", [2, 130])
def test_es_gradient_of_equal_pairs_is_zero(P, es_off):
    """ANTITHETIC with equal coeff inside every pair: exactly 0, and not 0 once one pair differs."""
    env = _obs_after_reset(3, 1)
    es_off(env)
    packed = env.set_policy(_t(ref.random_layers(np.random.default_rng(0), _widths("R1", "clip"))), "clip")
    _es_on(env, P, 1, True)
    coeff = np.repeat(np.random.default_rng(1).standard_normal(P // 2).astype(np.float32), 2)
    assert not _np(env.policy_es_gradient(torch.from_numpy(coeff))).any()
    coeff[1] += 1.0
    g = _np(env.policy_es_gradient(torch.from_numpy(coeff)))
    _assert_same(g, -eref.es_epsilon([0], packed.numel(), SEED, GEN)[0], "c_0 - c_1 = -1: minus eps of draw 0")


# ---- ES off, and what ES leaves alone

@pytest.mark.parametrize("head", ["clip", "argmax"])
def test_es_off_is_todays_call(head, es_off):
    """Before ES, with ES off after on, and with kind CP_ES_OFF: cp_policy_act's bits are the same; for a single
    policy and for a population."""
    B, R, G = 130, 3, 5
    env = _obs_after_reset(B, R)
    es_off(env)
    rng = np.random.default_rng(8)
    widths = _widths("wide", head)
    for members in (_t(ref.random_layers(rng, widths, scale=1.5)), [_t(ref.random_layers(rng, widths, scale=1.5)) for _ in range(3)]):
        population = isinstance(members[0], list)
        env.set_policy(members, head, group=G if population else None)
        a0 = env.policy_act().clone()
        if not population:
            _es_on(env, 7, G)
            assert not np.array_equal(_np(env.policy_act()), _np(a0))
            env.set_policy_es(None)
            _same(env.policy_act(), a0, "off after on")
        p = abi.cp_policy_es()
        p.kind, p.population, p.group = abi.CP_ES_OFF, -1, -1     # OFF: nothing else is read
        native.check(env.h, env.lib.cp_set_policy_es(env.h, C.byref(p)), "cp_set_policy_es")
        _same(env.policy_act(), a0, "kind CP_ES_OFF")


@pytest.mark.parametrize("autoreset", [0, 1])
def test_step_and_rollout_unchanged_with_es_set(autoreset):
    """cp_step and cp_rollout ignore the policy and ES: the same bits with and without."""
    B, R, K = 64, 2, 12
    rng = np.random.default_rng(3)
    layers = _t(ref.random_layers(rng, (14 * R, 6, 10)))
    acts = torch.from_numpy(rng.integers(0, 5, (K, B, 2)).astype(np.int8)).cuda()
    outs = []
    for with_es in (False, True):
        env = _env(num_envs=B, action_repeats=R, seed=2, autoreset=autoreset, max_episode_len=5)
        if with_es:
            env.set_policy_es(16, 0.1, group=3)      # before set_policy: either order
            env.set_policy(layers, "argmax")
        env.reset()
        steps = [tuple(x.clone() for x in env.step(acts[k])) for k in range(4)]
        if with_es:
            env.policy_act()
            env.policy_es_gradient(torch.ones(16))
        roll = tuple(x.clone() for x in env.rollout(acts[4:]))
        outs.append((steps, roll, env.get_state()))
    for k in range(4):
        for x, y in zip(outs[0][0][k], outs[1][0][k]):
            _same(x, y, f"step {k}")
    for x, y in zip(outs[0][1], outs[1][1]):
        _same(x, y, "rollout")
    _same(outs[0][2], outs[1][2], "state")


def test_rejections():
    R, P = 2, 6
    lib = native.load()
    env = _env(num_envs=8, action_repeats=R)
    env.reset()
    layers = _t(ref.random_layers(np.random.default_rng(0), (14 * R, 6, 10)))
    es = abi.cp_policy_es()
    es.kind, es.flags, es.sigma, es.population, es.group = abi.CP_ES_BYTES4, abi.CP_ES_ANTITHETIC, 0.1, P, 1
    out = torch.zeros((P, 6 * 29 + 10 * 7), device="cuda")
    coeff = torch.ones(P, device="cuda")

    def rejected(rc, who, needle, h=env.h):
        assert rc != 0
        err = lib.cp_last_error(h)
        assert err.startswith(who + b": ") and needle in err, err

    def weights(lo, n):
        return lib.cp_policy_es_weights(env.h, lo, n, out.data_ptr(), None)

    def gradient(lo, n):
        return lib.cp_policy_es_gradient(env.h, lo, n, coeff.data_ptr(), out.data_ptr(), None)

    # ES off; then ES on without a policy
    env.set_policy(layers, "argmax")
    rejected(weights(0, P), b"cp_policy_es_weights", b"ES is off")
    rejected(gradient(0, P), b"cp_policy_es_gradient", b"ES is off")
    env.set_policy(None)
    assert lib.cp_set_policy_es(env.h, C.byref(es)) == 0
    rejected(weights(0, P), b"cp_policy_es_weights", b"no policy set")
    rejected(gradient(0, P), b"cp_policy_es_gradient", b"no policy set")
    # member ranges outside [0, P)
    env.set_policy(layers, "argmax")
    for who, call in ((b"cp_policy_es_weights", weights), (b"cp_policy_es_gradient", gradient)):
        for lo, n in ((-1, 2), (0, P + 1), (P, 1), (P - 1, 2), (0, 0), (2, -1)):
            rejected(call(lo, n), who, b"member range")
        assert call(0, P) == 0 and call(P - 1, 1) == 0
    # whatever cp_policy_es_check rejects, under cp_set_policy_es's name; the handle keeps its setting
    bad = abi.cp_policy_es.from_buffer_copy(es)
    bad.group = 0
    rejected(lib.cp_set_policy_es(env.h, C.byref(bad)), b"cp_set_policy_es", b"group must be >= 1")
    assert weights(0, P) == 0
    # a [P][F] policy while ES is on
    members = [layers, _t(ref.random_layers(np.random.default_rng(1), (14 * R, 6, 10)))]
    env.set_policy(members, "argmax", group=4)
    a = torch.zeros((8, 2), dtype=torch.int8, device="cuda")
    rejected(lib.cp_policy_act(env.h, env.obs.data_ptr(), None, a.data_ptr(), None), b"cp_policy_act", b"population")
    rejected(weights(0, P), b"cp_policy_es_weights", b"population")
    env.set_policy_es(None)
    assert lib.cp_policy_act(env.h, env.obs.data_ptr(), None, a.data_ptr(), None) == 0
    torch.cuda.synchronize()
    # fp64 handles, a negative env_id_offset
    f64 = _env(num_envs=4, action_repeats=R, precision=abi.CP_PRECISION_F64)
    rejected(lib.cp_set_policy_es(f64.h, C.byref(es)), b"cp_set_policy_es", b"fp32 only", f64.h)
    neg = _env(num_envs=4, action_repeats=R, env_id_offset=-4)
    rejected(lib.cp_set_policy_es(neg.h, C.byref(es)), b"cp_set_policy_es", b"env_id_offset >= 0", neg.h)
    assert lib.cp_set_policy_es(neg.h, None) == 0
