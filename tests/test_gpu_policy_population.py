"""Policy populations on the MI355X (cp_policy.population / group): P weight sets behind one handle, env i reading
member ((env_id_offset + i) / G) % P.  The expected values are tests/policy_ref.py's, `forward` and the heads
called once per member on that member's env rows.  Both kernels are covered: the wave-uniform path (G and the
offset multiples of 64: every wave of the lane-per-env kernel serves one member) and the member path (anything
else: one member run per wave), bit for bit wherever the contract fixes every rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, policy
from tests import policy_ref as ref
from tests.test_gpu_parity import _assert_same, _np
from tests.test_gpu_policy import _env, _obs_after_reset, _same, _t

pytestmark = pytest.mark.gpu


def _widths(ws, head):
    out = 4 if head in ("clip", "tanh") else 10
    return {"R1": (14, 7, 5, out), "R2": (28, 7, 5, out), "R3": (42, 7, 5, out), "wide": (42, 100, 100, 50, out),
            "w128": (42, 128, out)}[ws]


def _R(ws):
    return {"R1": 1, "R2": 2}.get(ws, 3)


def _members(rng, widths, P, scale=2.0):
    return [ref.random_layers(rng, widths, scale=scale) for _ in range(P)]


def _z(members, x, G, off=0):
    """The last layer's outputs per env: forward once per member, on that member's env rows."""
    mem = policy.member_of(off + np.arange(x.shape[0], dtype=np.int64), G, len(members))
    z = np.zeros((x.shape[0], members[0][-1][0].shape[0]), np.float32)
    for m in np.unique(mem):
        z[mem == m] = ref.forward(members[m], x[mem == m])
    return z, mem


def _check_both_heads(env, ws, G, P, seed):
    """CLIP + noise and ARGMAX of a population of P random members on env's obs against the restatement."""
    B = env.B
    x = _np(env.obs).reshape(B, -1)
    for head in ("clip", "argmax"):
        rng = np.random.default_rng(seed + (head == "clip"))
        members = _members(rng, _widths(ws, head), P, scale=1.5 if ws in ("wide", "w128") else 2.0)
        packed = env.set_policy([_t(m) for m in members], head, group=G)
        assert packed.shape == (P, env.lib.cp_policy_floats(C.byref(env.policy))) and env.policy.population == P
        z, mem = _z(members, x, G)
        if head == "clip":
            noise = rng.uniform(-0.5, 0.5, (B, 2, 2)).astype(np.float32)
            _assert_same(_np(env.policy_act(noise=torch.from_numpy(noise))), ref.act_clip(z, noise), "clip + noise")
        else:
            _assert_same(_np(env.policy_act()), ref.act_argmax(z), "argmax")
        env.set_policy(None)
    return mem


@pytest.mark.parametrize("ws", ["R1", "R2", "R3", "wide"])
def test_wave_uniform_path_bit_exact(ws):
    """G = 64, P = 3, B = 200: four waves, the last partial, the members wrapping 0, 1, 2, 0."""
    env = _obs_after_reset(200, _R(ws))
    mem = _check_both_heads(env, ws, 64, 3, seed=400 + len(ws))
    assert mem[::64].tolist() == [0, 1, 2, 0]


@pytest.mark.parametrize("B", [3, 33, 130])
@pytest.mark.parametrize("P", [2, 7, "B"])
@pytest.mark.parametrize("G", [1, 5, 32, 96])
@pytest.mark.parametrize("ws", ["R1", "R2", "R3", "wide", "w128"])
def test_member_path_bit_exact(ws, G, P, B):
    """G = 96 is >= 64 and no multiple of 64 (runs cut into two chunks); G = 5 makes the runs straddle the
    lane-per-env kernel's wave boundaries; w128 is a layer with two units per lane."""
    P = B if P == "B" else P
    env = _obs_after_reset(B, _R(ws))
    _check_both_heads(env, ws, G, P, seed=1000 * G + 10 * P + B)


@pytest.mark.parametrize("head", ["clip", "argmax"])
def test_the_two_paths_agree(head):
    """192 envs at offset 0 with G = 64 take the wave-uniform path; 128 envs at env_id_offset = 32 with the same
    P, G and weights are misaligned, hence on the member path: given rows 32 .. 159 of the first handle's obs
    they return rows 32 .. 159 of its actions, raw bits."""
    R, P, G = 3, 3, 64
    rng = np.random.default_rng(23)
    members = [_t(m) for m in _members(rng, _widths("wide", head), P, scale=1.5)]
    whole = _obs_after_reset(192, R)
    whole.set_policy(members, head, group=G)
    noise = torch.from_numpy(rng.uniform(-0.5, 0.5, (192, 2, 2)).astype(np.float32)) if head == "clip" else None
    a = whole.policy_act(noise=noise).clone()
    obs = whole.obs.clone()
    whole.set_policy(None)
    shard = _env(num_envs=128, action_repeats=R, seed=11, env_id_offset=32)
    shard.reset()
    shard.set_policy(members, head, group=G)
    b = shard.policy_act(obs=obs[32:160].contiguous(), noise=None if noise is None else noise[32:160].contiguous())
    _same(b, a[32:160], "the member path against the wave-uniform path")
    assert len(np.unique(_np(a).reshape(192, -1), axis=0)) > 1   # not a constant answer


def test_sample_population():
    """G = 8, P = 5, B = 64: the epsilon draws exact, the others inside check_sample's interval with its DELTA;
    two handles of 32 envs at offsets 0 and 32 draw what the handle of 64 draws."""
    B, R, G, P, eps, seed = 64, 2, 8, 5, 0.25, (9 << 32) | 4
    rng = np.random.default_rng(31)
    raw = _members(rng, (14 * R, 7, 5, 10), P, scale=1.0)
    members = [_t(m) for m in raw]
    whole = _env(num_envs=B, action_repeats=R, seed=6)
    whole.reset()
    st = _np(whole.get_state())
    ints = abi.state_ints(st)
    ints[abi.CP_SF_STEPS] = rng.integers(0, 100, B)
    ints[abi.CP_SF_EPISODE] = rng.integers(0, 1000, B)
    steps, episode = ints[abi.CP_SF_STEPS].copy(), ints[abi.CP_SF_EPISODE].copy()
    whole.set_state(torch.from_numpy(st))
    whole.set_policy(members, "sample", epsilon=eps, seed=seed, group=G)
    obs = whole.obs.clone()
    z, mem = _z(raw, _np(obs).reshape(B, -1), G)
    assert len(np.unique(mem)) == P and mem[40] == 0          # the members wrap inside the batch
    a64 = _np(whole.policy_act())
    n_eps, n_soft, near = ref.check_sample(z, a64, ref.sample_words(steps, episode, np.arange(B), seed), eps)
    assert n_eps > 0 and n_soft > n_eps and near < 0.05
    parts = []
    for off in (0, 32):
        shard = _env(num_envs=32, action_repeats=R, seed=6, env_id_offset=off)
        shard.reset()
        shard.set_state(torch.from_numpy(np.ascontiguousarray(st[:, off:off + 32])))
        shard.set_policy(members, "sample", epsilon=eps, seed=seed, group=G)
        parts.append(_np(shard.policy_act(obs=obs[off:off + 32].contiguous())))
    assert np.array_equal(np.concatenate(parts), a64), "shards of 32 against one handle of 64"


@pytest.mark.parametrize("G,B", [(5, 33), (96, 130)])
def test_tanh_on_the_member_path(G, B):
    """|a - float32(tanh64(z))| <= 1e-6: the bound and its derivation are test_policy_act_tanh's (z is exact in
    the restatement, tanhf is OCML's: <= 5 ulp, one fp32 ulp in [-1, 1] <= 6e-8)."""
    R, P = 3, 7
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(G)
    raw = _members(rng, (14 * R, 7, 5, 4), P, scale=6.0)
    env.set_policy([_t(m) for m in raw], "tanh", group=G)
    z, _ = _z(raw, _np(env.obs).reshape(B, -1), G)
    a = _np(env.policy_act()).reshape(B, 4)
    err = np.abs(a.astype(np.float64) - np.tanh(z.astype(np.float64)).astype(np.float32).astype(np.float64)).max()
    print(f"tanh head, member path: max |a - tanh64(z)| = {err:.3g}, |z| up to {np.abs(z).max():.3g}")
    assert err <= 1e-6
    assert np.abs(z).max() > 0.5 and np.abs(a).max() <= 1.0
    noise = rng.uniform(-1.0, 1.0, (B, 2, 2)).astype(np.float32)
    an = _np(env.policy_act(noise=torch.from_numpy(noise))).reshape(B, 4)
    assert np.abs(an - np.clip(np.tanh(z.astype(np.float64)) + noise.reshape(B, 4), -1.0, 1.0)).max() <= 1e-6
    env.set_policy(None)


@pytest.mark.parametrize("head", ["clip", "sample"])
@pytest.mark.parametrize("G,B", [(64, 130), (5, 33)], ids=["wave-uniform", "member"])
def test_done_envs_get_zero_actions(G, B, head):
    """Done envs (a done field set through set_state: single envs inside a member run, and one whole run of
    G = 5) get 0 under both action kinds; the other envs of the same runs get the restatement's values."""
    R, P, eps, seed = 2, 2, 0.25, 5
    env = _env(num_envs=B, action_repeats=R, seed=3, autoreset=0)
    env.reset()
    st = _np(env.get_state())
    ints = abi.state_ints(st)
    done = np.zeros(B, bool)
    done[[1, 7, 12, B - 1]] = True
    done[20:25] = True                                   # with G = 5: every env of one member run
    ints[abi.CP_SF_DONE][done] = 1
    env.set_state(torch.from_numpy(st))
    rng = np.random.default_rng(21)
    raw = _members(rng, (14 * R, 7, 5, 4 if head == "clip" else 10), P)
    env.set_policy([_t(m) for m in raw], head, epsilon=eps, seed=seed, group=G)
    z, _ = _z(raw, _np(env.obs).reshape(B, -1), G)
    noise = rng.uniform(0.3, 0.5, (B, 2, 2)).astype(np.float32) if head == "clip" else None
    a = _np(env.policy_act(noise=None if noise is None else torch.from_numpy(noise)))
    assert not a[done].any(), "a done env's action is 0"
    if head == "clip":          # the noise alone keeps every evaluated action off 0
        _assert_same(a[~done], ref.act_clip(z, noise)[~done], "live envs")
        assert np.abs(a[~done]).min() > 0
    else:
        w = ref.sample_words(ints[abi.CP_SF_STEPS], ints[abi.CP_SF_EPISODE], np.arange(B), seed)
        ref.check_sample(z[~done], a[~done], w[~done], eps)


@pytest.mark.parametrize("G,B", [(64, 200), (5, 33)], ids=["wave-uniform", "member"])
def test_member_weights_are_read_live(G, B):
    """Member m's row overwritten in place (policy.repack on the row view): at the next policy_act exactly the
    envs of member m change, to the restatement's new values; all others keep their bits."""
    R, P, m = 2, 3, 1
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(12)
    raw = _members(rng, (14 * R, 7, 5, 4), P, scale=0.05)   # small: no output saturates at the clip
    packed = env.set_policy([_t(x) for x in raw], "clip", group=G)
    x = _np(env.obs).reshape(B, -1)
    z1, mem = _z(raw, x, G)
    a1 = _np(env.policy_act()).copy()
    _assert_same(a1, ref.act_clip(z1), "first weights")
    ptr = packed.data_ptr()
    raw[m] = ref.random_layers(rng, (14 * R, 7, 5, 4), scale=0.05)
    policy.repack(packed[m], _t(raw[m]))
    assert packed.data_ptr() == ptr and packed.shape == (P, 7 * 29 + 5 * 8 + 4 * 6)
    a2 = _np(env.policy_act())
    _assert_same(a2, ref.act_clip(_z(raw, x, G)[0]), "overwritten member")
    _assert_same(a2[mem != m], a1[mem != m], "the other members' envs")
    changed = (a2.reshape(B, -1) != a1.reshape(B, -1)).any(axis=1)
    assert changed[mem == m].all() and (mem == m).any() and (mem != m).any()
    env.set_policy(None)


@pytest.mark.parametrize("population", [0, 1])
def test_population_0_and_1_are_todays_call(population):
    """population 0 and 1 (group unread) give, bit for bit, what the same weights give through set_policy."""
    B, R = 33, 3
    env = _obs_after_reset(B, R)
    rng = np.random.default_rng(8)
    layers = _t(ref.random_layers(rng, (14 * R, 100, 50, 10), scale=1.5))
    env.set_policy(layers, "argmax")
    a0 = env.policy_act().clone()
    env.set_policy(None)
    packed, pol = policy.pack(layers, "argmax", device=env.device)
    pol.population, pol.group = population, -7
    native.check(env.h, env.lib.cp_set_policy(env.h, C.byref(pol)), "cp_set_policy")
    a = torch.zeros((B, 2), dtype=torch.int8, device=env.device)
    native.check(env.h, env.lib.cp_policy_act(env.h, env.obs.data_ptr(), None, a.data_ptr(), None), "cp_policy_act")
    torch.cuda.synchronize()
    _same(a, a0, f"population {population}")
    native.check(env.h, env.lib.cp_set_policy(env.h, None), "cp_set_policy")


@pytest.mark.parametrize("autoreset", [0, 1])
def test_step_and_rollout_unchanged_with_a_population_set(autoreset):
    """cp_step and cp_rollout ignore a policy, a population included: the same bits with and without one."""
    B, R, K = 64, 2, 12
    rng = np.random.default_rng(3)
    members = [_t(m) for m in _members(rng, (14 * R, 6, 10), 4)]
    acts = torch.from_numpy(rng.integers(0, 5, (K, B, 2)).astype(np.int8)).cuda()
    outs = []
    for with_policy in (False, True):
        env = _env(num_envs=B, action_repeats=R, seed=2, autoreset=autoreset, max_episode_len=5)
        if with_policy:
            env.set_policy(members, "argmax", group=5)
        env.reset()
        steps = [tuple(x.clone() for x in env.step(acts[k])) for k in range(4)]
        if with_policy:
            env.policy_act()
        roll = tuple(x.clone() for x in env.rollout(acts[4:]))
        outs.append((steps, roll, env.get_state()))
    for k in range(4):
        for x, y in zip(outs[0][0][k], outs[1][0][k]):
            _same(x, y, f"step {k}")
    for x, y in zip(outs[0][1], outs[1][1]):
        _same(x, y, "rollout")
    _same(outs[0][2], outs[1][2], "state")


def test_set_policy_population_rejections():
    R = 2
    rng = np.random.default_rng(0)
    members = [_t(m) for m in _members(rng, (14 * R, 6, 10), 3)]
    packed, pol = policy.pack_population(members, "argmax", group=4)
    env = _env(num_envs=8, action_repeats=R)
    lib = native.load()

    def rejected(needle, population, group):
        bad = abi.cp_policy.from_buffer_copy(pol)
        bad.population, bad.group = population, group
        assert lib.cp_set_policy(env.h, C.byref(bad)) != 0
        err = lib.cp_last_error(env.h)
        assert err.startswith(b"cp_set_policy: ") and needle in err, err

    rejected(b"population must be >= 0", -1, 4)
    rejected(b"group must be >= 1", 3, 0)
    rejected(b"group must be >= 1", 3, -64)
    # a rejected call leaves the handle without a policy; the accepted one works
    env.reset()
    a = torch.zeros((8, 2), dtype=torch.int8, device="cuda")
    assert lib.cp_policy_act(env.h, env.obs.data_ptr(), None, a.data_ptr(), None) != 0
    assert lib.cp_set_policy(env.h, C.byref(pol)) == 0
    # set_policy: a list of modules is a population, group defaulting to equal blocks of the handle
    seqs = [torch.nn.Sequential(torch.nn.Linear(14 * R, 6), torch.nn.ReLU(), torch.nn.Linear(6, 10)) for _ in range(2)]
    w = env.set_policy(seqs, "argmax")
    assert w.shape == (2, 6 * (14 * R + 1) + 10 * 7) and env.policy.population == 2 and env.policy.group == 4
    assert env.policy_act().shape == (8, 2)
    with pytest.raises(ValueError, match="one architecture"):
        env.set_policy([seqs[0], torch.nn.Sequential(torch.nn.Linear(14 * R, 10))], "argmax")
