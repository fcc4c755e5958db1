"""Returns and advantages on the MI355X (cp_returns_compute): the raw outputs bit for bit against the numpy
restatement (tests/returns_ref.py), the standardised ones within the derived bound, degenerate members,
determinism, shard invariance, split windows, the env's own episode returns, the rejections, and cp_step /
cp_rollout / cp_policy_act unchanged around a call.  The shapes are the smallest at which a walk can go wrong:
K around the 8-step register block, B around a wave, and B past one reduction slice (8,192 envs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, returns
from cartpoleplusplus_amd.batched import BatchedCartpole
from tests import policy_ref as pref
from tests import returns_ref as rr
from tests.test_gpu_policy import _env, _same, _t

pytestmark = pytest.mark.gpu
f32 = np.float32
GAMMA, LAM = 0.97, 0.9
PATTERNS = ("sparse", "none", "all", "last")
# (head, done_in, tail) given or not: none, all, and each alone
OPTIONALS = ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1))


def _data(K, B, pattern, seed):
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1.0, 2.0, (K, B)).astype(f32)
    if pattern == "sparse":
        done = (rng.random((K, B)) < 0.15).astype(np.uint8)
    elif pattern == "none":
        done = np.zeros((K, B), np.uint8)
    elif pattern == "all":
        done = np.ones((K, B), np.uint8)
    else:
        done = np.zeros((K, B), np.uint8)
        done[K - 1] = 1
    return dict(reward=reward, done=done, values=rng.normal(0.0, 3.0, (K + 1, B)).astype(f32),
                head=rng.uniform(0.5, 9.0, B).astype(f32), done_in=(rng.random(B) < 0.3).astype(np.uint8),
                tail=rng.normal(0.0, 3.0, B).astype(f32))


def _cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _both(d, kind, boundary, opt=(1, 1, 1), mask_open=False, **kw):
    """(library, restatement) raw outputs for the data d."""
    head, done_in, tail = (d[n] if on else None for n, on in zip(("head", "done_in", "tail"), opt))
    values = d["values"] if kind == rr.GAE else None
    got = returns.advantages(_cuda(d["reward"]), _cuda(d["done"]), kind, gamma=GAMMA, lam=LAM, values=_cuda(values),
                             head=_cuda(head), done_in=_cuda(done_in), tail=_cuda(tail), boundary=boundary,
                             mask_open=mask_open, **kw)
    want = rr.raw(d["reward"], d["done"], kind, boundary, GAMMA, LAM, values, head, done_in, tail, mask_open)
    return got, want


def _assert_raw(got, want, what):
    adv, valid, carry, ret = want
    assert np.array_equal(_np(got.valid), valid), f"{what}: valid"
    assert np.array_equal(_np(got.adv).view(np.uint32), adv.view(np.uint32)), f"{what}: adv"
    assert np.array_equal(_np(got.carry).view(np.uint32), carry.view(np.uint32)), f"{what}: carry"
    assert (got.ret is None) == (ret is None), f"{what}: ret"
    if ret is not None:
        assert np.array_equal(_np(got.ret).view(np.uint32), ret.view(np.uint32)), f"{what}: ret"


# ---- raw parity

@pytest.mark.parametrize("boundary", rr.BOUNDARIES)
@pytest.mark.parametrize("kind", rr.KINDS)
def test_raw_outputs_bit_exact(kind, boundary):
    n = 0
    for K in (1, 2, 7, 19):
        for B in (1, 3, 64, 65, 130):
            for pi, pattern in enumerate(PATTERNS):
                d = _data(K, B, pattern, 1000 * K + 10 * B + pi)
                for oi, opt in enumerate(OPTIONALS):
                    mask_open = (K + B + pi + oi) % 2 == 1
                    got, want = _both(d, kind, boundary, opt, mask_open)
                    _assert_raw(got, want, f"K={K} B={B} {pattern} head/done_in/tail={opt} mask_open={mask_open}")
                    n += 1
    assert n == 4 * 5 * 4 * 5


@pytest.mark.parametrize("kind,boundary", list(zip(rr.KINDS, rr.BOUNDARIES)))
def test_raw_outputs_bit_exact_200x4096(kind, boundary):
    d = _data(200, 4096, "sparse", 5)
    if kind == rr.EPISODE_TOTAL:        # long episodes too: some envs close one only late in the window
        d["done"][:, ::3] &= (np.arange(200) % 77 == 76).astype(np.uint8)[:, None]
    got, want = _both(d, kind, boundary, mask_open=True)
    _assert_raw(got, want, f"{kind} {boundary}")
    assert want[1].min() == 0 and want[1].max() == 1


# ---- standardised parity

def _assert_standardised(d, kind, boundary, P, G, off, what):
    B = d["reward"].shape[1]
    _, raw = _both(d, kind, boundary, env_id_offset=off, population=P, group=G)
    got, _ = _both(d, kind, boundary, standardise=True, env_id_offset=off, population=P, group=G)
    assert np.array_equal(_np(got.valid), raw[1]), f"{what}: valid"
    assert np.array_equal(_np(got.carry).view(np.uint32), raw[2].view(np.uint32)), f"{what}: carry"
    if raw[3] is not None:              # ret is never standardised
        assert np.array_equal(_np(got.ret).view(np.uint32), raw[3].view(np.uint32)), f"{what}: ret"
    ref_out, stats = rr.standardise(raw[0], raw[1], off, P, G)
    mem = rr.members(B, off, P, G)
    g_stats = _np(got.stats)
    assert g_stats.shape == (max(P, 1), 4)
    assert np.array_equal(g_stats[:, 0], stats[:, 0]), f"{what}: n"
    assert np.array_equal(g_stats[:, 3], stats[:, 3]), f"{what}: degenerate"
    live = stats[:, 3] == 0
    n = stats[live, 0]
    scale = np.abs(raw[0]).max() + np.abs(stats[live, 1])
    assert (np.abs(g_stats[live, 1] - stats[live, 1]) <= n * 2.0 ** -52 * scale).all(), f"{what}: mean"
    assert (np.abs(g_stats[live, 2] - stats[live, 2]) <= 4 * n * 2.0 ** -52 * scale ** 2 / stats[live, 2]).all(), \
        f"{what}: std"
    if live.any():                        # not vacuous: a live member's outputs have unit variance
        assert np.abs(ref_out).max() > 0.5 and np.abs(_np(got.adv)).max() > 0.5
    bound = rr.standardise_bound(ref_out, raw[0], raw[1], stats, mem)
    err = np.abs(_np(got.adv).astype(np.float64) - ref_out.astype(np.float64))
    worst = (err / np.maximum(bound, 1e-300)).max()
    print(f"{what}: max |out - ref| / bound = {worst:.3g}")
    assert (err <= bound).all(), f"{what}: {worst:.3g} of the bound"
    return stats, g_stats


@pytest.mark.parametrize("off", [0, 37, (1 << 32) + 5])
@pytest.mark.parametrize("kind", rr.KINDS)
def test_standardised_within_the_derived_bound(kind, off):
    K, B = 19, 130
    for bi, boundary in enumerate(rr.BOUNDARIES):
        d = _data(K, B, "sparse", 77 + bi)
        for P, G in ((1, 1), (2, 1), (7, 5), (B, 1), (3, 100)):     # (3, 100): runs longer than the call is wide
            _assert_standardised(d, kind, boundary, P, G, off, f"{kind} {boundary} P={P} G={G} off={off}")
    d = _data(7, 3, "last", 9)                                       # P * G wider than the call
    _assert_standardised(d, kind, rr.SAME_STEP, 7, 5, off, f"{kind} B=3 P=7 G=5 off={off}")


@pytest.mark.parametrize("P,G", [(1, 1), (2, 1), (3, 4100)])
def test_standardised_past_one_reduction_slice(P, G):
    """B > 8,192: a member's envs are reduced in more than one slice."""
    d = _data(3, 2 * 8192 + 77, "sparse", 21)
    _assert_standardised(d, rr.DISCOUNTED, rr.SAME_STEP, P, G, 37, f"B=16461 P={P} G={G}")


def test_episode_total_of_integer_rewards_has_the_exact_mean():
    K, B = 19, 130
    d = _data(K, B, "sparse", 31)
    d["reward"] = np.ones((K, B), f32)               # the env's own rewards
    for P, G, off in ((1, 1, 0), (7, 5, 37), (2, 1, (1 << 32) + 5)):
        stats, g_stats = _assert_standardised(d, rr.EPISODE_TOTAL, rr.SAME_STEP, P, G, off, f"P={P} G={G} off={off}")
        assert np.array_equal(g_stats[:, 1], stats[:, 1]) and (stats[:, 0] > 0).all()


# ---- further cases

def test_degenerate_members_get_zeros_and_the_flag():
    K, B = 12, 6
    reward = np.ones((K, B), f32)
    done = np.zeros((K, B), np.uint8)
    done[3::4] = 1                                    # every episode totals 4: "converged?"
    done[:, 2] = 0
    done[5, 2] = done[11, 2] = 1                      # env 2 (member 1): totals 6 and 6 ... and env 3: 4
    done[:, 4:] = 0                                   # member 2 (envs 4, 5): no episode closes, no valid sample
    got = returns.advantages(_cuda(reward), _cuda(done), standardise=True, population=3, group=2)
    raw = rr.raw(reward, done)
    ref_out, stats = rr.standardise(raw[0], raw[1], 0, 3, 2)
    assert list(stats[:, 3]) == [1, 0, 1] and list(stats[:, 0]) == [24, 24, 0]
    g_stats = _np(got.stats)
    assert np.array_equal(g_stats, stats)
    adv = _np(got.adv)
    assert not adv[:, :2].any() and not adv[:, 4:].any()
    assert np.array_equal(adv[:, 2:4], ref_out[:, 2:4]) and list(adv[0, 2:4]) == [1, -1]
    assert np.array_equal(_np(got.valid), raw[1]) and not raw[1][:, 4:].any()
    # all totals equal and one member for all: lrpg's converged case
    got = returns.advantages(_cuda(reward[:, :2]), _cuda(done[:, :2]), standardise=True)
    assert not _np(got.adv).any() and list(_np(got.stats)[0]) == [24, 4, 0, 1] and _np(got.valid).all()


@pytest.mark.parametrize("kind", rr.KINDS)
def test_two_equal_calls_give_equal_bits(kind):
    d = _data(19, 2 * 8192 + 77, "sparse", 3)
    outs = [_both(d, kind, rr.NEXT_STEP, standardise=True, env_id_offset=37, population=5, group=3)[0] for _ in range(2)]
    for a, b, name in zip(outs[0], outs[1], outs[0]._fields):
        if a is not None:
            _same(a, b, name)


@pytest.mark.parametrize("kind", rr.KINDS)
def test_raw_outputs_do_not_depend_on_the_sharding(kind):
    d = _data(19, 64, "sparse", 4)
    whole, _ = _both(d, kind, rr.NEXT_STEP, env_id_offset=0, population=3, group=5)
    for lo in (0, 32):
        part = {k: np.ascontiguousarray(v[..., lo:lo + 32]) for k, v in d.items()}
        got, _ = _both(part, kind, rr.NEXT_STEP, env_id_offset=lo, population=3, group=5)
        for a, b, name in zip(got, whole, got._fields):
            if a is not None:
                _same(a, b[..., lo:lo + 32], f"{name} at offset {lo}")


@pytest.mark.parametrize("boundary", rr.BOUNDARIES)
def test_split_windows_chain_through_carry_and_done_in(boundary):
    K, B = 12, 130
    d = _data(K, B, "sparse", 8)
    if boundary == rr.STICKY:             # what a handle without autoreset returns: done stays, reward 0 after it
        seen = np.maximum.accumulate(d["done"], axis=0)
        d["reward"][1:] = np.where(seen[:-1] != 0, f32(0), d["reward"][1:])
        d["done"] = seen
    reward, done = _cuda(d["reward"]), _cuda(d["done"])
    one = returns.advantages(reward, done, boundary=boundary)
    w1 = returns.advantages(reward[:6].contiguous(), done[:6].contiguous(), boundary=boundary)
    w2 = returns.advantages(reward[6:].contiguous(), done[6:].contiguous(), boundary=boundary, head=w1.carry,
                            done_in=done[5].contiguous())
    a, v = _np(one.adv), _np(one.valid)
    a1, v1, a2, v2 = _np(w1.adv), _np(w1.valid), _np(w2.adv), _np(w2.valid)
    assert (v1 <= v[:6]).all() and np.array_equal(a1[v1 != 0].view(np.uint32), a[:6][v1 != 0].view(np.uint32))
    # the second window sees everything the single call saw of its steps, the episodes crossing the cut included
    assert np.array_equal(v2, v[6:]) and np.array_equal(a2.view(np.uint32), a[6:].view(np.uint32))
    _same(w2.carry, one.carry, "carry")
    crossing = (v[:6] != 0) & (v1 == 0)     # steps of episodes that cross the cut: open in the first window
    assert crossing.any() and (v2 != 0).any()


def _collect(env, K, seed):
    """K random-action steps into preallocated (K, B) buffers."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    reward = torch.empty((K, env.B), device=env.device, dtype=torch.float32)
    done = torch.empty((K, env.B), device=env.device, dtype=torch.uint8)
    for k in range(K):
        a = (torch.rand((env.B, 2, 2), generator=g) * 2 - 1).to(env.device)
        _, r, dn = env.step(a)
        reward[k].copy_(r)
        done[k].copy_(dn)
    return reward, done


def test_sticky_totals_are_the_envs_own_episode_returns():
    env = BatchedCartpole(130, autoreset=False, done_on_bounds=True)
    env.reset()
    reward, done = _collect(env, 40, 1)
    out = env.advantages(reward, done)
    ret, length = env.episode_returns()
    adv, valid, carry, dn = _np(out.adv), _np(out.valid), _np(out.carry), _np(done)
    ret, length = _np(ret), _np(length)
    finished = dn[-1] != 0
    print(f"{finished.sum()} of 130 envs finished within 40 steps")
    assert finished.any() and not finished.all()
    for i in range(130):
        if finished[i]:
            first = int(np.argmax(dn[:, i] != 0))
            assert length[i] == first + 1
            assert valid[:first + 1, i].all() and not valid[first + 1:, i].any()      # the later samples are padding
            assert (adv[:first + 1, i].view(np.uint32) == ret[i:i + 1].view(np.uint32)).all()
            assert not adv[first + 1:, i].any() and carry[i] == 0
        else:
            assert not valid[:, i].any() and not adv[:, i].any() and carry[i] == 40.0
    want = rr.raw(_np(reward), dn, rr.EPISODE_TOTAL, rr.STICKY)
    _assert_raw(out, want, "sticky, the env's own window")


def test_same_step_totals_with_max_episode_len_5():
    env = BatchedCartpole(130, autoreset=True, max_episode_len=5)
    env.reset()
    reward, done = _collect(env, 12, 2)
    out = env.advantages(reward, done)
    adv, valid, carry = _np(out.adv), _np(out.valid), _np(out.carry)
    assert (adv[:10] == 5.0).all() and valid[:10].all()
    assert not adv[10:].any() and not valid[10:].any()              # the open tail
    assert (carry == 2.0).all()
    ret, length = env.episode_returns()
    assert (_np(ret) == 5.0).all() and (_np(length) == 5).all()
    std = env.advantages(reward, done, standardise=True)            # all totals equal: degenerate
    assert not _np(std.adv).any() and list(_np(std.stats)[0]) == [1300, 5, 0, 1]


def test_env_advantages_takes_the_handles_population():
    B, R = 130, 1
    env = _env(num_envs=B, action_repeats=R, seed=3, autoreset=1, max_episode_len=4, env_id_offset=37)
    rng = np.random.default_rng(0)
    d = _data(9, B, "sparse", 12)
    reward, done = _cuda(d["reward"]), _cuda(d["done"])
    assert _np(env.advantages(reward, done, standardise=True).stats).shape == (1, 4)
    env.set_policy(_t(pref.random_layers(rng, (14 * R, 5, 4))), "clip")
    env.set_policy_es(7, 0.1, group=5)
    got = env.advantages(reward, done, standardise=True)
    want = returns.advantages(reward, done, standardise=True, population=7, group=5, env_id_offset=37)
    for a, b, name in zip(got, want, got._fields):
        if a is not None:
            _same(a, b, name)
    assert _np(got.stats).shape == (7, 4)
    env.set_policy_es(None)
    env.set_policy([[(torch.from_numpy(W), torch.from_numpy(b)) for W, b in pref.random_layers(rng, (14 * R, 5, 4))]
                    for _ in range(3)], "clip", group=4)
    got = env.advantages(reward, done, "discounted", gamma=0.9, standardise=True)
    want = returns.advantages(reward, done, "discounted", gamma=0.9, standardise=True, population=3, group=4,
                              env_id_offset=37)
    _same(got.adv, want.adv, "population of the policy")
    assert _np(got.stats).shape == (3, 4)
    # without autoreset the boundary is sticky
    env2 = _env(num_envs=B, action_repeats=R, seed=3, autoreset=0)
    _same(env2.advantages(reward, done).adv, returns.advantages(reward, done, boundary="sticky").adv, "sticky")


# ---- rejections

def test_compute_rejections():
    lib = native.load()
    K, B = 4, 8
    f = torch.zeros((K + 1, B), device="cuda")
    u = torch.zeros((K, B), device="cuda", dtype=torch.uint8)
    s = torch.zeros(4096, device="cuda", dtype=torch.uint8)

    def call(kind=abi.CP_RET_EPISODE_TOTAL, reward=f, done=u, values=None, adv=f, valid=u, ret=None, scratch=s, **kw):
        p = abi.cp_returns()
        p.kind, p.gamma, p.lam, p.steps, p.num_envs, p.population, p.group = kind, 1.0, 1.0, K, B, 1, 1
        for k, v in kw.items():
            setattr(p, k, v)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = lib.cp_returns_compute(C.byref(p), ptr(reward), ptr(done), ptr(values), None, None, None, ptr(adv),
                                    ptr(valid), None, ptr(ret), None, ptr(scratch), None)
        return rc, lib.cp_last_error(None)

    out = torch.empty((K, B), device="cuda")
    assert call(adv=out)[0] == 0
    for kw in (dict(reward=None), dict(done=None), dict(adv=None), dict(valid=None), dict(scratch=None)):
        rc, err = call(**kw)
        assert rc < 0 and b"null reward, done, adv_out, valid_out or scratch" in err, (kw, err)
    rc, err = call(kind=abi.CP_RET_GAE, adv=out)
    assert rc < 0 and b"needs values" in err
    rc, err = call(kind=abi.CP_RET_DISCOUNTED, adv=out, ret=out)
    assert rc < 0 and b"ret_out is CP_RET_GAE's output" in err
    assert call(kind=abi.CP_RET_GAE, values=f, adv=out, ret=torch.empty((K, B), device="cuda"))[0] == 0
    rc, err = call(adv=out, steps=0)
    assert rc < 0 and b"steps must be >= 1" in err
    rc, err = call(adv=out, scratch=s[1:])
    assert rc < 0 and b"16-byte aligned" in err
    torch.cuda.synchronize()


def test_wrapper_rejects_wrong_dtype_shape_device_and_layout():
    K, B = 6, 10
    reward = torch.ones((K, B), device="cuda")
    done = torch.zeros((K, B), device="cuda", dtype=torch.uint8)
    ok = returns.advantages(reward, done)
    assert ok.ret is None and ok.stats is None and tuple(ok.adv.shape) == (K, B)
    bad = [
        (dict(reward=reward.double()), "reward: expected dtype"),
        (dict(done=done.bool()), "done: expected dtype"),
        (dict(done=done.float()), "done: expected dtype"),
        (dict(done=done[:, :5].contiguous()), "done: expected shape"),
        (dict(reward=reward[0]), "reward: expected a (K, B)"),
        (dict(reward=reward.cpu()), "reward: expected a GPU tensor"),
        (dict(done=done.cpu()), "done: expected device"),
        (dict(reward=reward.t().contiguous().t()), "reward: must be contiguous"),
        (dict(done=torch.zeros((K, 2 * B), device="cuda", dtype=torch.uint8)[:, ::2]), "done: must be contiguous"),
        (dict(head=torch.ones(B, device="cuda", dtype=torch.float64)), "head: expected dtype"),
        (dict(head=torch.ones(B + 1, device="cuda")), "head: expected shape"),
        (dict(done_in=torch.ones(B, device="cuda")), "done_in: expected dtype"),
        (dict(tail=torch.ones((1, B), device="cuda")), "tail: expected shape"),
        (dict(kind="gae"), "needs values"),
        (dict(kind="gae", values=torch.ones((K, B), device="cuda")), "values: expected shape"),
        (dict(values=torch.ones((K + 1, B), device="cuda")), "values is for kind 'gae'"),
        (dict(kind="td"), "kind must be one of"),
        (dict(boundary="soft"), "boundary must be one of"),
        (dict(reward=np.ones((K, B), f32)), "reward: expected a (K, B)"),
    ]
    for kw, msg in bad:
        args = dict(reward=reward, done=done)
        args.update(kw)
        with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            returns.advantages(**args)
    with pytest.raises(native.CartpoleError, match="gamma must be finite"):
        returns.advantages(reward, done, "discounted", gamma=1.5)
    with pytest.raises(native.CartpoleError, match="group must be >= 1"):
        returns.advantages(reward, done, standardise=True, population=4, group=0)


# ---- the env's own entry points are untouched

def test_step_rollout_and_policy_act_unchanged_around_a_call():
    B, R = 64, 2
    rng = np.random.default_rng(3)
    layers = _t(pref.random_layers(rng, (14 * R, 6, 4)))
    acts = torch.from_numpy(rng.uniform(-1, 1, (3, B, 2, 2)).astype(f32)).cuda()
    d = _data(7, B, "sparse", 2)
    outs = []
    for interleave in (False, True):
        env = _env(num_envs=B, action_repeats=R, seed=2, autoreset=1, max_episode_len=4)
        env.set_policy(layers, "tanh")
        env.reset()
        log = []
        for k in range(3):
            if interleave:
                env.advantages(_cuda(d["reward"]), _cuda(d["done"]), "gae", values=_cuda(d["values"]), gamma=GAMMA,
                               lam=LAM, standardise=True)
            a = env.policy_act()
            log.append(a.clone())
            log.extend(x.clone() for x in env.step(a))
            log.append(env.terminal_obs.clone())
        if interleave:
            env.advantages(_cuda(d["reward"]), _cuda(d["done"]), standardise=True, population=3, group=2)
        log.extend(x.clone() for x in env.rollout(acts))
        log.append(env.get_state())
        outs.append(log)
    assert len(outs[0]) == len(outs[1]) == 3 * 5 + 3 + 1
    for n, (x, y) in enumerate(zip(*outs)):
        _same(x, y, f"output {n}")
