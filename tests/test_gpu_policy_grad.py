"""cp_policy_gradient on the MI355X against tests/policy_grad_ref.py: the logits bit for bit (the contract pins the
forward pass), logp and the gradient within the bounds derived from the fp32 formats (policy_grad_ref.logp_bound /
grad_bound), the exact properties (determinism, skipped samples, heads, sharding, live weights), an ascent step, the
rejections and the absence of side effects.  Each test prints its largest error / bound ratio before asserting."""
import ctypes as C

import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi, native, policy
from tests import policy_grad_ref as gref
from tests import policy_ref as ref
from tests.test_gpu_policy import _env, _t

pytestmark = pytest.mark.gpu

ARCH = {"7,5": (7, 5), "100,50": (100, 50), "none": (), "128x3": (128, 128, 128)}
BIG = (1 << 32) + 5
# (architecture, R, K, B, P, G, env_id_offset): every value of the issue's table, and every pair that takes
# another path (runs cut by the handle's ends, one env per member, tiles of several steps, three-layer wide nets
# at 32 samples per tile)
CASES = [
    ("7,5", 1, 1, 1, 1, 1, 0), ("7,5", 3, 2, 3, 1, 1, 37), ("7,5", 1, 7, 64, 2, 1, 0), ("7,5", 3, 7, 65, 3, 5, 37),
    ("7,5", 1, 2, 130, "B", 1, BIG), ("7,5", 3, 1, 130, 2, 64, 0), ("7,5", 1, 7, 3, "B", 1, 0),
    ("7,5", 3, 7, 64, 2, 64, 37), ("7,5", 1, 1, 65, 3, 5, BIG),
    ("100,50", 3, 7, 130, 1, 1, 0), ("100,50", 3, 2, 65, 2, 1, 37), ("100,50", 1, 7, 64, 3, 5, BIG),
    ("100,50", 3, 1, 130, 2, 64, 37), ("100,50", 3, 2, 3, "B", 1, 0), ("100,50", 1, 1, 1, 1, 1, BIG),
    ("none", 1, 7, 65, 1, 1, 0), ("none", 3, 2, 130, 3, 5, 37), ("none", 1, 1, 1, 1, 1, BIG), ("none", 3, 7, 64, "B", 1, 0),
    ("128x3", 3, 2, 65, 2, 1, 0), ("128x3", 1, 7, 130, 2, 64, BIG), ("128x3", 3, 1, 3, 1, 1, 37),
    ("128x3", 1, 2, 64, 3, 5, 37),
]


def _widths(arch, R):
    return (14 * R,) + ARCH[arch] + (10,)


def _data(rng, K, B, nin, skip=True):
    obs = rng.standard_normal((K, B, nin)).astype(np.float32)
    act = rng.integers(0, 5, (K, B, 2)).astype(np.int8)
    coeff = rng.standard_normal((K, B)).astype(np.float32)
    if skip and K * B >= 4:
        n = K * B
        coeff.reshape(-1)[rng.choice(n, max(1, n // 5), replace=False)] = 0.0
        coeff.reshape(-1)[rng.integers(n)] = -0.0
        bad = rng.choice(n, max(1, n // 16), replace=False)
        act.reshape(-1, 2)[bad, rng.integers(0, 2, len(bad))] = rng.choice(np.array([-1, 5, 9, 127, -128], np.int8), len(bad))
    return obs, act, coeff


def _setup(env, members, P, G, head="sample", epsilon=0.1):
    if P > 1:
        env.set_policy([_t(m) for m in members], head, epsilon=epsilon, seed=3, group=G)
    else:
        env.set_policy(_t(members[0]), head, epsilon=epsilon, seed=3)


def _call(env, obs, act, coeff):
    K = obs.shape[0]
    g, lp, lg = env.policy_gradient(torch.from_numpy(obs).cuda().view(K, env.B, env.R, 2, 7), torch.from_numpy(act).cuda(),
                                    torch.from_numpy(coeff).cuda(), logp=True, logits=True)
    torch.cuda.synchronize()
    return g.cpu().numpy().reshape(max(env.policy.population, 1), -1), lp.cpu().numpy(), lg.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check(got, want, widths, what):
    """got = (grad, logp, logits) of the library, want = policy_grad_ref.window(...)."""
    g, lp, lg = got
    assert np.array_equal(_bits(lg), _bits(want["logits"])), what + ": logits bits"
    err = np.abs(lp.astype(np.float64) - want["logp"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r_lp = np.where(want["bound_logp"] > 0, err / want["bound_logp"], np.where(err > 0, np.inf, 0.0)).max()
    r_g = 0.0
    for m in range(g.shape[0]):
        bound = gref.grad_bound(widths, int(want["n"][m]), want["absscale"][m])
        e = np.abs(g[m].astype(np.float64) - want["grad"][m])
        assert not g[m][want["absscale"][m] == 0].any(), f"{what}: member {m} non-zero where absscale is 0"
        nz = bound > 0
        if nz.any():
            r_g = max(r_g, float((e[nz] / bound[nz]).max()))
    print(f"{what}: logp err/bound {r_lp:.3f}, grad err/bound {r_g:.3f}")
    assert r_lp <= 1.0, f"{what}: logp error {r_lp:.3f} of its bound"
    assert r_g <= 1.0, f"{what}: gradient error {r_g:.3f} of its bound"
    return r_lp, r_g


@pytest.mark.parametrize("arch,R,K,B,P,G,off", CASES)
def test_against_the_reference(arch, R, K, B, P, G, off):
    P = B if P == "B" else P
    widths = _widths(arch, R)
    rng = np.random.default_rng([len(arch), R, K, B, P, G, off % 1000])
    members = [ref.random_layers(rng, widths, scale=1.5) for _ in range(P)]
    obs, act, coeff = _data(rng, K, B, widths[0])
    env = _env(num_envs=B, action_repeats=R, env_id_offset=off)
    _setup(env, members, P, G)
    got = _call(env, obs, act, coeff)
    want = gref.window(members, obs, act, coeff, P, G, off)
    _check(got, want, widths, f"{arch} R={R} K={K} B={B} P={P} G={G} off={off}")
    again = _call(env, obs, act, coeff)
    for a, b in zip(got, again):
        assert np.array_equal(_bits(a), _bits(b)), "two equal calls give equal bits"


def _partials(env, K):
    P = max(env.policy.population, 1)
    F = env.lib.cp_policy_floats(C.byref(env.policy))
    bytes_ = env.lib.cp_policy_gradient_scratch_bytes(env.h, K)
    assert bytes_ > 0 and bytes_ % 16 == 0
    return -(-bytes_ // (P * F * 4))


def test_several_partials_per_member():
    """K = 40, B = 130, P = 2, G = 1: 65 one-env runs of one tile each per member, so the documented scratch formula
    shows more than one partial; a member's partials are added in order."""
    K, B, P, G, R = 40, 130, 2, 1, 1
    widths = _widths("7,5", R)
    rng = np.random.default_rng(40)
    members = [ref.random_layers(rng, widths, scale=1.5) for _ in range(P)]
    obs, act, coeff = _data(rng, K, B, widths[0])
    env = _env(num_envs=B, action_repeats=R)
    _setup(env, members, P, G)
    assert _partials(env, K) > 1
    assert _partials(env, 1) >= 1
    _check(_call(env, obs, act, coeff), gref.window(members, obs, act, coeff, P, G, 0), widths, "several partials")


def test_exact_properties():
    K, B, P, G, R = 7, 65, 3, 5, 3
    widths = _widths("100,50", R)
    rng = np.random.default_rng(77)
    members = [ref.random_layers(rng, widths, scale=1.5) for _ in range(P)]
    obs, act, coeff = _data(rng, K, B, widths[0])
    env = _env(num_envs=B, action_repeats=R)
    _setup(env, members, P, G, "sample", 0.1)
    base = _call(env, obs, act, coeff)
    # all-zero coeff: an all-zero grad, logp and logits
    for z in _call(env, obs, act, np.zeros_like(coeff)):
        assert not z.any()
    # skipped samples' obs NaN and their actions 9: the same bits
    ev = gref.evaluated(act, coeff).reshape(K, B)
    obs2, act2 = obs.copy(), act.copy()
    obs2[~ev] = np.nan
    act2[~ev] = 9
    assert (~ev).sum() > 10
    for a, b in zip(base, _call(env, obs2, act2, coeff)):
        assert np.array_equal(_bits(a), _bits(b)), "skipped samples are not read"
    # ARGMAX against SAMPLE, and another epsilon
    for head, eps in (("argmax", 0.0), ("sample", 0.7)):
        _setup(env, members, P, G, head, eps)
        for a, b in zip(base, _call(env, obs, act, coeff)):
            assert np.array_equal(_bits(a), _bits(b)), f"{head} epsilon {eps}"
    # a member without samples: only envs of members 0 and 2 carry a coeff
    mem = gref.members(B, P, G, 0)
    c3 = coeff.copy()
    c3[:, mem == 1] = 0.0
    g3 = _call(env, obs, act, c3)[0]
    assert not g3[1].any() and g3[0].any() and g3[2].any()
    # live weights: new weights written in place are what the next call differentiates
    members2 = [ref.random_layers(rng, widths, scale=1.0) for _ in range(P)]
    env.policy_weights.copy_(torch.from_numpy(np.stack([ref.packed(m) for m in members2])))
    _check(_call(env, obs, act, coeff), gref.window(members2, obs, act, coeff, P, G, 0), widths, "live weights")


def test_two_shards_against_one_handle():
    """Two handles of 32 envs at offsets 0 and 32 against one of 64: logits and logp bit for bit, the summed grads
    within the gradient bound."""
    K, P, G, R = 7, 3, 5, 1
    widths = _widths("7,5", R)
    rng = np.random.default_rng(64)
    members = [ref.random_layers(rng, widths, scale=1.5) for _ in range(P)]
    obs, act, coeff = _data(rng, K, 64, widths[0])
    whole = _env(num_envs=64, action_repeats=R)
    _setup(whole, members, P, G)
    gw, lpw, lgw = _call(whole, obs, act, coeff)
    want = gref.window(members, obs, act, coeff, P, G, 0)
    _check((gw, lpw, lgw), want, widths, "one handle of 64")
    gs = np.zeros_like(gw, dtype=np.float64)
    for off in (0, 32):
        shard = _env(num_envs=32, action_repeats=R, env_id_offset=off)
        _setup(shard, members, P, G)
        sl = slice(off, off + 32)
        g, lp, lg = _call(shard, np.ascontiguousarray(obs[:, sl]), np.ascontiguousarray(act[:, sl]),
                          np.ascontiguousarray(coeff[:, sl]))
        assert np.array_equal(_bits(lp), _bits(lpw[:, sl])) and np.array_equal(_bits(lg), _bits(lgw[:, sl]))
        gs += g.astype(np.float64)
    for m in range(P):
        bound = gref.grad_bound(widths, int(want["n"][m]), want["absscale"][m])
        assert (np.abs(gs[m] - want["grad"][m]) <= bound).all()


def test_logits_are_what_policy_act_acts_on():
    B, R = 130, 3
    widths = _widths("100,50", R)
    rng = np.random.default_rng(9)
    members = [ref.random_layers(rng, widths, scale=1.5) for _ in range(3)]
    for P, G in ((1, 1), (3, 5), (2, 64)):
        env = _env(num_envs=B, action_repeats=R, seed=11)
        env.reset()
        _setup(env, members[:P], P, G, "argmax", 0.0)
        acts = env.policy_act()
        lg = env.policy_gradient(env.obs.unsqueeze(0), acts.unsqueeze(0), torch.ones((1, B), device="cuda"), logits=True)[1]
        assert torch.equal(lg.view(B, 2, 5).argmax(-1).to(torch.int8), acts)
        x = env.obs.cpu().numpy().reshape(1, B, -1)
        want = gref.window(members[:P], x, acts.cpu().numpy()[None], np.ones((1, B), np.float32), P, G, 0)
        assert np.array_equal(_bits(lg.cpu().numpy()), _bits(want["logits"]))


def _objective(lp, coeff):
    return float((coeff.astype(np.float64) * lp.astype(np.float64)).sum())


def test_an_ascent_step_does_not_decrease_the_objective():
    """w += lr * grad on random nets with K * B = 260 samples, the seeds chosen on the CPU so that the reference's
    own gradient step raises the reference's objective."""
    K, B, R, lr = 4, 65, 1, 1e-4
    widths = _widths("7,5", R)
    found = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        layers = ref.random_layers(rng, widths, scale=1.0)
        obs, act, coeff = _data(rng, K, B, widths[0])
        w0 = gref.window([layers], obs, act, coeff)
        stepped = (ref.packed(layers) + np.float32(lr) * w0["grad"][0].astype(np.float32)).astype(np.float32)
        layers1 = [(W.numpy().copy(), b.numpy().copy()) for W, b in
                   policy.unpack(torch.from_numpy(stepped), list(widths))]
        w1 = gref.window([layers1], obs, act, coeff)
        if not (coeff * w1["logp"]).sum() > (coeff * w0["logp"]).sum():
            continue
        found += 1
        env = _env(num_envs=B, action_repeats=R)
        _setup(env, [layers], 1, 1)
        g, lp0, _ = _call(env, obs, act, coeff)
        env.policy_weights.add_(lr * torch.from_numpy(g[0]).cuda())
        lp1 = _call(env, obs, act, coeff)[1]
        print(f"seed {seed}: objective {_objective(lp0, coeff):.6f} -> {_objective(lp1, coeff):.6f}")
        assert _objective(lp1, coeff) >= _objective(lp0, coeff)
        if found == 3:
            break
    assert found == 3


def test_rejections():
    B, R = 8, 1
    widths = _widths("7,5", R)
    rng = np.random.default_rng(3)
    layers = ref.random_layers(rng, widths)
    obs, act, coeff = (torch.from_numpy(x).cuda() for x in _data(rng, 2, B, 14, skip=False))
    obs = obs.view(2, B, R, 2, 7)
    env = _env(num_envs=B, action_repeats=R)
    lib, VP = env.lib, C.c_void_p
    with pytest.raises(native.CartpoleError, match="no policy set"):
        env.policy_gradient(obs, act, coeff)
    assert lib.cp_policy_gradient_scratch_bytes(env.h, 2) < 0 and b"no policy set" in lib.cp_last_error(env.h)
    cont = ref.random_layers(rng, (14, 7, 5, 4))
    for head in ("tanh", "clip"):
        env.set_policy(_t(cont), head)
        with pytest.raises(native.CartpoleError, match="continuous head"):
            env.policy_gradient(obs, act, coeff)
    env.set_policy(_t(layers), "sample")
    env.set_policy_es(4, sigma=0.1)
    with pytest.raises(native.CartpoleError, match="ES perturbations are on"):
        env.policy_gradient(obs, act, coeff)
    env.set_policy_es(None)
    grad, _ = env.policy_gradient(obs, act, coeff, logp=True)        # allocates the wrapper's scratch
    F = grad.numel()
    scratch = torch.empty(lib.cp_policy_gradient_scratch_bytes(env.h, 2) + 16, device="cuda", dtype=torch.uint8)
    p = dict(obs=obs.data_ptr(), actions=act.data_ptr(), coeff=coeff.data_ptr(), grad=grad.data_ptr(), scratch=scratch.data_ptr())

    def call(steps=2, **kw):
        q = dict(p, **kw)
        return lib.cp_policy_gradient(env.h, steps, VP(q["obs"]), VP(q["actions"]), VP(q["coeff"]), None, None,
                                      VP(q["grad"]), VP(q["scratch"]), None)

    for steps in (0, -1):
        assert call(steps=steps) < 0 and b"steps must be >= 1" in lib.cp_last_error(env.h)
        assert lib.cp_policy_gradient_scratch_bytes(env.h, steps) < 0
    assert call(steps=(1 << 31) - 1) < 0 and b"below 2^31" in lib.cp_last_error(env.h)
    assert lib.cp_policy_gradient_scratch_bytes(env.h, (1 << 31) - 1) < 0
    for name in p:
        assert call(**{name: None}) < 0 and b"null obs, actions, coeff, grad_out or scratch" in lib.cp_last_error(env.h), name
    assert call(scratch=scratch.data_ptr() + 4) < 0 and b"16-byte aligned" in lib.cp_last_error(env.h)
    assert call() == 0 and F == lib.cp_policy_floats(C.byref(env.policy))
    # the wrapper's own checks
    with pytest.raises(ValueError, match="obs"):
        env.policy_gradient(obs[:, :4], act, coeff)
    with pytest.raises(ValueError, match="actions"):
        env.policy_gradient(obs, act[:1], coeff)
    with pytest.raises(ValueError, match="actions"):
        env.policy_gradient(obs, act.float(), coeff)
    with pytest.raises(ValueError, match="coeff"):
        env.policy_gradient(obs, act, coeff.view(-1))
    g2 = env.policy_gradient(obs.cpu(), act.cpu(), coeff.t().contiguous().t())   # moved / made contiguous, as _device_buffer does
    torch.cuda.synchronize()
    assert torch.equal(g2, grad)


def test_no_side_effects():
    """Two equal handles, one with gradient calls between its other calls: the same actions, obs, rewards and state."""
    B, R, K = 65, 2, 3
    widths = _widths("7,5", R)
    rng = np.random.default_rng(12)
    layers = ref.random_layers(rng, widths, scale=2.0)
    obs, act, coeff = (torch.from_numpy(x).cuda() for x in _data(rng, K, B, widths[0]))
    obs = obs.view(K, B, R, 2, 7)
    envs = [_env(num_envs=B, action_repeats=R, seed=5, autoreset=abi.CP_AUTORESET_SAME_STEP) for _ in range(2)]
    out = []
    for e, with_grad in zip(envs, (False, True)):
        e.reset()
        _setup(e, [layers], 1, 1, "sample", 0.2)
        rec = []
        s0 = e.get_state().view(torch.int32).clone()      # raw bits: the counters are integers in float fields
        if with_grad:
            e.policy_gradient(obs, act, coeff)
            assert torch.equal(e.get_state().view(torch.int32), s0)
        a = e.policy_act().clone()
        if with_grad:
            e.policy_gradient(obs, act, coeff)
        rec += [a] + [t.clone() for t in e.step(a)]
        if with_grad:
            e.policy_gradient(obs, act, coeff)
        ro = e.rollout(torch.from_numpy(np.random.default_rng(1).integers(0, 5, (4, B, 2)).astype(np.int8)).cuda())
        rec += [t.clone() for t in ro] + [e.get_state().view(torch.int32).clone()]
        out.append(rec)
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_captured_into_a_graph():
    """The call in a captured graph ("100,50": more than 64 KiB of LDS per block): a replay after new weights were
    written in place gives the bits of an eager call on those weights."""
    K, B, R = 3, 65, 3
    widths = _widths("100,50", R)
    rng = np.random.default_rng(21)
    layers, layers2 = (ref.random_layers(rng, widths, scale=s) for s in (1.5, 1.0))
    obs, act, coeff = (torch.from_numpy(x).cuda() for x in _data(rng, K, B, widths[0]))
    obs = obs.view(K, B, R, 2, 7)
    env = _env(num_envs=B, action_repeats=R)
    _setup(env, [layers], 1, 1)
    first = [t.clone() for t in env.policy_gradient(obs, act, coeff, logp=True)]   # eager: the scratch exists now
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            captured = env.policy_gradient(obs, act, coeff, logp=True)
    torch.cuda.current_stream().wait_stream(stream)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, first):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    env.policy_weights.copy_(torch.from_numpy(ref.packed(layers2)))
    g.replay()
    torch.cuda.synchronize()
    eager = env.policy_gradient(obs, act, coeff, logp=True)
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(captured[0], first[0])
    del g
