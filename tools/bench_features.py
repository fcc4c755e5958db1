"""Cost of the §8f rows on top of the C3 step at full size (one MI355X):
    base    env.step (C3: B=65,536, R=3, discrete, autoreset)
    lqr     env.step with the in-kernel LQR policy + 8-state readback (f4)
    ingest  env.step + ReplayMemory.after_step (f3; 2^22-event ring, 42-float states)
    sample  ReplayMemory.sample(n) alone (device gather)
Timed with HIP events on torch's current stream (all launches go there).  Prints one
JSON line; per-event / per-sample algorithmic bytes as in DESIGN.md §Replay memory.

--policy: the in-kernel MLP policy instead, one session, K = --steps env-steps per run,
one warm-up run and the median of --repeats runs each:
    rollout         cp_rollout with precomputed actions (the yardstick)
    act_loop        K x (cp_policy_act + cp_step), "100,50" MLP with the SAMPLE head
    torch_loop      what a user does without it: K x (torch MLP forward + torch.multinomial + cp_step)

--policy --population [LEGS]: the policy-population legs instead, same net, head and sizes:
    a  P = 1                      b  P = 1,024, G = 64 (wave-uniform path)     c  P = 16, G = 4,096 (wave-uniform)
    d  P = B = 65,536, G = 1 (member path)                                      e  P = 2,048, G = 32 (member path)
cp_policy_act alone over K launches per run for every leg, and the closed loop K x (cp_policy_act + cp_step) for
a, b and d; d and e also against the weight-streaming floor P * F * 4 bytes / --copy-tbps.  Leg a uses nothing
newer than set_policy / policy_act, so `--tree OTHER_CHECKOUT --population a` times another build of the library
with the same code (the P = 1 gate: run the two alternately in one session).  --out writes the JSON to a file.

--policy --noise [LEGS]: the exploration-noise legs (DESIGN.md §9.5 "Exploration noise"): ddpg's actor
("100,100,50", TANH head) with OU noise at the agent's defaults, at B = 4,096 with R = 2 (C2) and at B = 65,536:
    off     cp_policy_act alone, noise off (nothing newer than set_policy / policy_act, so `--tree OTHER_CHECKOUT
            --noise off` times the parent build: the noise-off gate, the two builds alternating in one session)
    kernel  K x (policy_act with in-kernel OU + step)
    torch   K x (the caller's torch OU update of INTEGRATION.md + policy_act(noise=x) + step)

--policy --es [LEGS]: the seeded ES perturbation legs (DESIGN.md §9.5 "ES perturbations"; es_bench below).

--returns: returns and advantages of a rollout window (DESIGN.md §9.5 "Returns and advantages"; returns_bench below).

--policy-gradient: cp_policy_gradient against today's torch update (DESIGN.md §9.5 "Policy gradient";
policy_gradient_bench below)."""
import argparse
import json
import os
import sys

import torch

_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_TREE))
from cartpoleplusplus_amd.batched import BatchedCartpole  # noqa: E402
from cartpoleplusplus_amd.lqr import exact_gains  # noqa: E402
from cartpoleplusplus_amd.replay_memory import ReplayMemory  # noqa: E402


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for t in range(steps):
        fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def policy_bench(args):
    import statistics
    B, K, R = args.batch, args.steps, 3
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    acts = torch.randint(0, 5, (K, B, 2), dtype=torch.int8, device=dev, generator=g)
    mlp = torch.nn.Sequential(torch.nn.Linear(14 * R, 100), torch.nn.ReLU(), torch.nn.Linear(100, 50), torch.nn.ReLU(),
                              torch.nn.Linear(50, 10)).to(dev)
    env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
    env.set_policy(mlp, "sample", epsilon=0.05, seed=7)
    env.reserve_rollout(K, terminal=False)
    env.reset()

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def torch_loop():
        with torch.no_grad():
            for _ in range(K):
                logits = mlp(env.obs.view(B, -1)).view(B * 2, 5)
                a = torch.multinomial(torch.softmax(logits, 1), 1).view(B, 2).to(torch.int8)
                env.step(a)

    legs = {"rollout": lambda: env.rollout(acts, terminal=False),
            "act_loop": lambda: [env.step(env.policy_act()) for _ in range(K)],
            "torch_loop": torch_loop}
    out = {"batch": B, "steps": K, "repeats": args.repeats, "policy": "42-100-50-10 sample"}
    for name, fn in legs.items():
        run(fn)  # warm-up
        ms = [run(fn) for _ in range(args.repeats)]
        out[name + "_ms"] = ms
        out[name + "_env_steps_per_s"] = B * K / (statistics.median(ms) * 1e-3)
    out["act_loop_over_rollout"] = out["act_loop_env_steps_per_s"] / out["rollout_env_steps_per_s"]
    out["act_loop_over_torch_loop"] = out["act_loop_env_steps_per_s"] / out["torch_loop_env_steps_per_s"]
    print(json.dumps(out))


POPULATION_LEGS = {"a": (1, None), "b": (1024, 64), "c": (16, 4096), "d": (None, 1), "e": (2048, 32)}   # (P, G); None: B


def population_bench(args):
    import statistics
    B, K, R = args.batch, args.steps, 3
    dev = torch.device("cuda", 0)
    widths = (14 * R, 100, 50, 10)
    F = sum(o * (i + 1) for i, o in zip(widths[:-1], widths[1:]))
    env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
    env.reset()

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def series(fn):
        run(fn)  # warm-up
        ms = [run(fn) for _ in range(args.repeats)]
        med = statistics.median(ms)
        return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med}

    out = {"tree": os.path.abspath(_TREE), "batch": B, "steps": K, "repeats": args.repeats,
           "policy": "42-100-50-10 sample", "floats_per_member": F, "copy_tbps": args.copy_tbps, "legs": {}}
    for leg in args.population.split(","):
        P, G = POPULATION_LEGS[leg]
        P = B if P is None else P
        g = torch.Generator(device=dev).manual_seed(1234 + P)
        if P == 1:
            layers = [(torch.randn((o, i), device=dev, generator=g) / i ** 0.5, torch.randn((o,), device=dev, generator=g) * 0.1)
                      for i, o in zip(widths[:-1], widths[1:])]
            env.set_policy(layers, "sample", epsilon=0.05, seed=7)
        else:
            stacked = [(torch.randn((P, o, i), device=dev, generator=g) / i ** 0.5,
                        torch.randn((P, o), device=dev, generator=g) * 0.1) for i, o in zip(widths[:-1], widths[1:])]
            env.set_policy(stacked, "sample", epsilon=0.05, seed=7, group=G)
            del stacked
        res = {"population": P, "group": G, "weight_bytes": P * F * 4}
        res["act"] = series(lambda: [env.policy_act() for _ in range(K)])
        res["act_us_per_launch"] = res["act"]["median_ms"] * 1e3 / K
        if leg in ("a", "b", "d"):
            env.reset()
            res["act_step_loop"] = series(lambda: [env.step(env.policy_act()) for _ in range(K)])
            res["act_step_loop_env_steps_per_s"] = B * K / (res["act_step_loop"]["median_ms"] * 1e-3)
        if leg in ("d", "e"):   # the member path streams every member's weights once per launch
            res["floor_us"] = P * F * 4 / (args.copy_tbps * 1e12) * 1e6
            res["floor_fraction"] = res["floor_us"] / res["act_us_per_launch"]
        env.set_policy(None)
        out["legs"][leg] = res
    if "a" in out["legs"]:
        for leg, res in out["legs"].items():
            res["act_over_leg_a"] = res["act_us_per_launch"] / out["legs"]["a"]["act_us_per_launch"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


ES_LEGS = {"anti": (None, 1, True), "plain": (None, 1, False), "g8": (8192, 8, True)}   # (P, G, antithetic); None: B


def es_bench(args):
    """--policy --es [LEGS]: seeded ES perturbations (DESIGN.md §9.5 "ES perturbations"), the population legs' net,
    head and sizes.  anti / plain / g8: cp_policy_act alone and the closed loop with ES on; d: the materialised
    [P][F] population of the same members (P = B, G = 1: the population legs' leg (d)) as the yardstick; grad:
    policy_es_gradient at P = B against the einsum over kept noise tensors."""
    import statistics
    B, K, R = args.batch, args.steps, 3
    dev = torch.device("cuda", 0)
    widths = (14 * R, 100, 50, 10)
    F = sum(o * (i + 1) for i, o in zip(widths[:-1], widths[1:]))
    sigma = 0.05
    env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
    env.reset()
    g = torch.Generator(device=dev).manual_seed(1234)
    layers = [(torch.randn((o, i), device=dev, generator=g) / i ** 0.5, torch.randn((o,), device=dev, generator=g) * 0.1)
              for i, o in zip(widths[:-1], widths[1:])]

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def series(fn):
        run(fn)  # warm-up
        ms = [run(fn) for _ in range(args.repeats)]
        med = statistics.median(ms)
        return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med}

    def act_and_loop(res):
        res["act"] = series(lambda: [env.policy_act() for _ in range(K)])
        res["act_us_per_launch"] = res["act"]["median_ms"] * 1e3 / K
        env.reset()
        res["act_step_loop"] = series(lambda: [env.step(env.policy_act()) for _ in range(K)])
        res["act_step_loop_env_steps_per_s"] = B * K / (res["act_step_loop"]["median_ms"] * 1e-3)

    out = {"tree": os.path.abspath(_TREE), "batch": B, "steps": K, "repeats": args.repeats,
           "policy": "42-100-50-10 sample", "floats_per_member": F, "sigma": sigma, "legs": {}}
    for leg in args.es.split(","):
        if leg in ES_LEGS:
            P, G, anti = ES_LEGS[leg]
            P = B if P is None else P
            env.set_policy(layers, "sample", epsilon=0.05, seed=7)
            env.set_policy_es(P, sigma, group=G, seed=11, antithetic=anti)
            # the centre, and the gradient's slices (64 x F floats, the library's) : all the ES path holds
            res = {"population": P, "group": G, "antithetic": anti, "device_bytes": F * 4 + 64 * F * 4}
            act_and_loop(res)
        elif leg == "d":
            env.set_policy(layers, "sample", epsilon=0.05, seed=7)
            env.set_policy_es(B, sigma, group=1, seed=11)
            W = env.policy_es_weights()
            env.set_policy_es(None)
            env.set_policy(_stacked(W, widths), "sample", epsilon=0.05, seed=7, group=1)
            del W
            # the [P][F] weights, and the [P][F] noise the caller keeps for the update
            res = {"population": B, "group": 1, "device_bytes": 2 * B * F * 4}
            act_and_loop(res)
        elif leg == "grad":
            env.set_policy(layers, "sample", epsilon=0.05, seed=7)
            env.set_policy_es(B, sigma, group=1, seed=11)
            fit = torch.randn((B,), device=dev, generator=g)
            res = {"population": B, "es_gradient": series(lambda: [env.policy_es_gradient(fit) for _ in range(10)])}
            res["es_gradient_us"] = res["es_gradient"]["median_ms"] * 1e3 / 10
            noise = [(torch.randn((B, o, i), device=dev, generator=g), torch.randn((B, o), device=dev, generator=g))
                     for i, o in zip(widths[:-1], widths[1:])]
            res["einsum"] = series(lambda: [[(torch.einsum("b,boi->oi", fit, nw), torch.einsum("b,bo->o", fit, nb))
                                             for nw, nb in noise] for _ in range(10)])
            res["einsum_us"] = res["einsum"]["median_ms"] * 1e3 / 10
            res["einsum_noise_bytes"] = B * F * 4
            del noise
        else:
            raise SystemExit(f"--es: unknown leg {leg!r} (anti, plain, g8, d, grad)")
        env.set_policy_es(None)
        env.set_policy(None)
        torch.cuda.empty_cache()
        out["legs"][leg] = res
    if "d" in out["legs"]:
        for leg, res in out["legs"].items():
            if "act_us_per_launch" in res:
                res["act_over_leg_d"] = res["act_us_per_launch"] / out["legs"]["d"]["act_us_per_launch"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _torch_advantages(reward, done, kind, gamma, lam, values, member, P):
    """What a user writes without the library call (SAME_STEP boundary): loops over k of elementwise ops (forwards
    for the episode totals, then backwards), and scatter_add for the per-member statistics in float64."""
    K, B = reward.shape
    d = done != 0
    adv = torch.zeros_like(reward)
    valid = torch.zeros_like(done)
    ret = None
    if kind == "episode_total":
        closing = torch.zeros_like(reward)
        T = torch.zeros_like(reward[0])
        for k in range(K):
            T = T + reward[k]
            closing[k] = T
            T = torch.where(d[k], torch.zeros_like(T), T)
        cur = torch.zeros_like(reward[0])
        closed = torch.zeros_like(d[0])
        for k in range(K - 1, -1, -1):
            closed = closed | d[k]
            cur = torch.where(d[k], closing[k], cur)
            adv[k] = torch.where(closed, cur, torch.zeros_like(cur))
            valid[k] = closed
    else:
        c = (torch.tensor(gamma, dtype=torch.float32) * torch.tensor(lam, dtype=torch.float32)).item()
        A = torch.zeros_like(reward[0])
        ret = torch.empty_like(reward)
        for k in range(K - 1, -1, -1):
            delta = (reward[k] + gamma * values[k + 1]) - values[k]
            A = torch.where(d[k], reward[k] - values[k], delta + c * A)
            adv[k] = A
            ret[k] = A + values[k]
        valid.fill_(1)
        return adv, valid, ret
    x = adv.double()
    v = (valid != 0).double()
    idx = member.expand(K, B).reshape(-1)
    n = torch.zeros(P, dtype=torch.float64, device=reward.device).scatter_add_(0, idx, v.reshape(-1))
    s1 = torch.zeros_like(n).scatter_add_(0, idx, (x * v).reshape(-1))
    mean = s1 / n.clamp(min=1)
    dev = (x - mean[member]) * v
    s2 = torch.zeros_like(n).scatter_add_(0, idx, (dev * dev).reshape(-1))
    std = (s2 / n.clamp(min=1)).sqrt()
    ok = (n > 0) & (std > 0)
    out = torch.where(ok[member], dev / std.clamp(min=1e-300)[member], torch.zeros_like(dev)).float()
    return out, valid, ret


def returns_bench(args):
    """--returns: cp_returns_compute (cartpoleplusplus_amd.returns.advantages) against the torch loop above, in one
    process on one build: K = --steps, at B = 65,536 with P = 1 and at B = 4,096 with P = 16, G = 256; the legs
    EPISODE_TOTAL + STANDARDISE and GAE.  us per call: one warm-up run and the median of --repeats runs (a run is
    `calls` back-to-back calls between two events), spread = max - min over the median.  Bytes per sample, the
    algorithm's: reward, done, adv, valid = 10; GAE adds values and ret, 8; standardisation adds a read of adv and
    valid (5) and a read of both with a write of adv (9)."""
    import statistics
    from cartpoleplusplus_amd import returns
    dev = torch.device("cuda", 0)
    K = args.steps
    gamma, lam = 0.99, 0.95

    def run(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    def series(fn, calls):
        run(fn, calls)  # warm-up
        us = [run(fn, calls) for _ in range(args.repeats)]
        med = statistics.median(us)
        return {"us": us, "median_us": med, "spread": (max(us) - min(us)) / med, "calls_per_run": calls}

    out = {"tree": os.path.abspath(_TREE), "steps": K, "repeats": args.repeats, "copy_tbps": args.copy_tbps,
           "device": torch.cuda.get_device_name(0), "gamma": gamma, "lam": lam, "boundary": "same_step", "sizes": {}}
    for B, P, G in ((65536, 1, 1), (4096, 16, 256)):
        g = torch.Generator(device=dev).manual_seed(1234 + B)
        reward = torch.ones((K, B), device=dev)
        # ragged episodes of about 50 steps, none longer than 120
        done = (torch.rand((K, B), device=dev, generator=g) < 0.02)
        done[119::120] = True
        done = done.to(torch.uint8)
        values = torch.randn((K + 1, B), device=dev, generator=g)
        member = (torch.arange(B, device=dev) // G) % P
        size = {"batch": B, "population": P, "group": G, "legs": {}}
        legs = {
            "episode_total_standardise": (
                lambda: returns.advantages(reward, done, standardise=True, population=P, group=G),
                lambda: _torch_advantages(reward, done, "episode_total", gamma, lam, None, member, P), 10 + 5 + 9),
            "gae": (
                lambda: returns.advantages(reward, done, "gae", gamma=gamma, lam=lam, values=values),
                lambda: _torch_advantages(reward, done, "gae", gamma, lam, values, member, P), 10 + 8),
        }
        for name, (lib_fn, torch_fn, bytes_per_sample) in legs.items():
            a, b = lib_fn(), torch_fn()
            err = (a.adv - b[0]).abs().max().item()      # the same function: the torch sums run in another order
            same_valid = bool((a.valid == b[1]).all().item())
            res = {"library": series(lib_fn, 20), "torch": series(torch_fn, 1), "max_abs_diff_to_torch": err,
                   "valid_equal": same_valid, "bytes_per_sample": bytes_per_sample}
            nbytes = bytes_per_sample * K * B
            res["algorithmic_bytes"] = nbytes
            res["library_tbps"] = nbytes / (res["library"]["median_us"] * 1e-6) / 1e12
            res["share_of_copy_bandwidth"] = res["library_tbps"] / args.copy_tbps
            res["torch_over_library"] = res["torch"]["median_us"] / res["library"]["median_us"]
            res["gate_library_not_slower"] = res["library"]["median_us"] <= res["torch"]["median_us"]
            size["legs"][name] = res
            del a, b
        out["sizes"][f"B{B}_P{P}"] = size
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["gate_library_not_slower"] and r["valid_equal"] for s in out["sizes"].values() for r in s["legs"].values()):
        raise SystemExit("--returns: the library call is slower than the torch loop, or disagrees with it")


def policy_gradient_bench(args):
    """--policy-gradient: BatchedCartpole.policy_gradient against the torch path it replaces (forward, loss, backward,
    repack on a torch mirror of the net), in one process on one build, at B = --batch, R = 3, K = --steps, lrpg's
    "100,50" net, the ragged valid mask of --returns' done pattern (coeff = the standardised episode totals, 0
    where invalid).  Legs: P = 1, and P = 16 with G = B / 16 (torch: one forward / backward / repack per member).
    ms per call: one warm-up run and the median of --repeats runs, spread = (max - min) / median; the peak allocated
    memory of each leg above what it starts with.  FLOPs 6 F N (N the evaluated samples: forward, dW and W^T delta,
    2 F each) against --fp32-tflops; bytes: the obs, actions and coeff read once, logp never written."""
    import statistics
    from cartpoleplusplus_amd import policy
    dev = torch.device("cuda", 0)
    B, K, R = args.batch, args.steps, 3
    widths = (14 * R, 100, 50, 10)
    F = sum(o * (i + 1) for i, o in zip(widths[:-1], widths[1:]))
    g = torch.Generator(device=dev).manual_seed(4321)

    def make_net():
        return torch.nn.Sequential(torch.nn.Linear(widths[0], 100), torch.nn.ReLU(), torch.nn.Linear(100, 50), torch.nn.ReLU(),
                                   torch.nn.Linear(50, 10)).to(dev)

    env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
    obs = torch.randn((K, B, R, 2, 7), device=dev, generator=g)
    act = torch.randint(0, 5, (K, B, 2), dtype=torch.int8, device=dev, generator=g)
    reward = torch.ones((K, B), device=dev)
    done = (torch.rand((K, B), device=dev, generator=g) < 0.02)
    done[119::120] = True
    done = done.to(torch.uint8)

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def series(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run(fn)  # warm-up
        ms = [run(fn) for _ in range(args.repeats)]
        med = statistics.median(ms)
        return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med,
                "peak_extra_bytes": torch.cuda.max_memory_allocated() - base}

    out = {"tree": os.path.abspath(_TREE), "batch": B, "steps": K, "repeats": args.repeats, "floats": F,
           "device": torch.cuda.get_device_name(0), "fp32_tflops": args.fp32_tflops, "copy_tbps": args.copy_tbps, "legs": {}}
    for P in (1, 16):
        G = B // P
        nets = [make_net() for _ in range(P)]
        if P == 1:
            env.set_policy(nets[0], "sample", epsilon=0.05, seed=7)
        else:
            env.set_policy(nets, "sample", epsilon=0.05, seed=7, group=G)
        adv = env.advantages(reward, done, standardise=True, population=P, group=G)
        coeff, valid = adv.adv, adv.valid.bool()
        N = int((coeff != 0).sum().item())
        rows = [env.policy_weights[m] if P > 1 else env.policy_weights for m in range(P)]

        def lib_fn():
            return env.policy_gradient(obs, act, coeff)

        def torch_fn():
            for m in range(P):
                sl = slice(m * G, (m + 1) * G)
                v = valid[:, sl]
                net = nets[m]
                net.zero_grad(set_to_none=True)
                logp = torch.log_softmax(net(obs[:, sl][v].reshape(-1, widths[0])).view(-1, 2, 5), -1)
                chosen = logp.gather(-1, act[:, sl][v].long().unsqueeze(-1)).squeeze(-1).sum(-1)
                loss = -(chosen * coeff[:, sl][v]).mean()
                loss.backward()
                policy.repack(rows[m], net)

        lib, tor = series(lib_fn), series(torch_fn)
        # the same function: -n_m * the mean loss's gradient is the library's sum
        gl = lib_fn().reshape(P, -1)
        torch_fn()
        gt = torch.stack([-float(valid[:, m * G:(m + 1) * G].sum().item()) * torch.cat(
            [t.grad.reshape(-1) for lin in nets[m] if isinstance(lin, torch.nn.Linear) for t in (lin.weight, lin.bias)])
            for m in range(P)])
        leg = {"population": P, "group": G, "evaluated_samples": N, "library": lib, "torch": tor,
               "max_rel_diff_to_torch": ((gl - gt).abs().max() / gt.abs().max()).item(),
               "scratch_bytes": int(env.lib.cp_policy_gradient_scratch_bytes(env.h, K))}
        leg["torch_over_library"] = tor["median_ms"] / lib["median_ms"]
        leg["library_tflops"] = 6.0 * F * N / (lib["median_ms"] * 1e-3) / 1e12
        leg["share_of_fp32_peak"] = leg["library_tflops"] / args.fp32_tflops
        nbytes = N * (widths[0] * 4) + K * B * (2 + 4)
        leg["algorithmic_bytes"] = nbytes
        leg["library_tbps"] = nbytes / (lib["median_ms"] * 1e-3) / 1e12
        leg["share_of_copy_bandwidth"] = leg["library_tbps"] / args.copy_tbps
        out["legs"][f"P{P}"] = leg
        del nets, gl, gt, adv
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _stacked(W, widths):
    """Packed rows (P, F) as a stacked population [(W (P, out, in), b (P, out)), ...]."""
    out, o = [], 0
    for i, n in zip(widths[:-1], widths[1:]):
        out.append((W[:, o:o + n * i].reshape(-1, n, i), W[:, o + n * i:o + n * i + n]))
        o += n * i + n
    return out


NOISE_SIZES = ((4096, 2), (65536, 3))   # (B, R): C2, and the full-size batch of the other policy legs


def noise_bench(args):
    """ddpg's actor ("100,100,50", TANH head, continuous actions) with OU exploration noise at the agent's
    defaults (theta = 0.01, sigma = 0.05), per size one handle, K = --steps per run, one warm-up run and the
    median of --repeats runs per leg."""
    import statistics
    K = args.steps
    dev = torch.device("cuda", 0)
    theta, sigma = 0.01, 0.05

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def series(fn):
        run(fn)  # warm-up
        ms = [run(fn) for _ in range(args.repeats)]
        med = statistics.median(ms)
        return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med}

    out = {"tree": os.path.abspath(_TREE), "steps": K, "repeats": args.repeats, "policy": "14R-100-100-50-4 tanh",
           "ou": {"theta": theta, "sigma": sigma}, "sizes": {}}
    for B, R in NOISE_SIZES:
        g = torch.Generator(device=dev).manual_seed(1234 + B)
        widths = (14 * R, 100, 100, 50, 4)
        layers = [(torch.randn((o, i), device=dev, generator=g) / i ** 0.5, torch.randn((o,), device=dev, generator=g) * 0.1)
                  for i, o in zip(widths[:-1], widths[1:])]
        env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
        env.set_policy(layers, "tanh")
        env.reset()
        res = {"action_repeats": R}
        for leg in args.noise.split(","):
            if leg == "off":        # cp_policy_act alone, no noise: nothing newer than set_policy / policy_act
                res["off_act"] = series(lambda: [env.policy_act() for _ in range(K)])
                res["off_act_us_per_launch"] = res["off_act"]["median_ms"] * 1e3 / K
            elif leg == "kernel":   # K x (policy_act with in-kernel OU + step)
                env.reset()
                env.set_policy_noise("ou", theta=theta, sigma=sigma, seed=7)
                res["kernel_act"] = series(lambda: [env.policy_act() for _ in range(K)])
                res["kernel_act_us_per_launch"] = res["kernel_act"]["median_ms"] * 1e3 / K
                res["kernel_loop"] = series(lambda: [env.step(env.policy_act()) for _ in range(K)])
                res["kernel_loop_env_steps_per_s"] = B * K / (res["kernel_loop"]["median_ms"] * 1e-3)
                env.set_policy_noise(None)
            elif leg == "torch":    # K x (the caller's torch OU update + policy_act(noise=x) + step)
                env.reset()
                x = [torch.zeros((B, 2, 2), device=dev)]

                def torch_loop():
                    for _ in range(K):
                        x[0] = x[0] + theta * (0.0 - x[0]) + sigma * torch.randn_like(x[0])
                        env.step(env.policy_act(noise=x[0]))
                res["torch_loop"] = series(torch_loop)
                res["torch_loop_env_steps_per_s"] = B * K / (res["torch_loop"]["median_ms"] * 1e-3)
            else:
                raise SystemExit(f"--noise: legs are off, kernel, torch; got {leg!r}")
        if "kernel_loop" in res and "torch_loop" in res:
            res["kernel_over_torch"] = res["kernel_loop_env_steps_per_s"] / res["torch_loop_env_steps_per_s"]
        out["sizes"][str(B)] = res
        env.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", action="store_true")
    ap.add_argument("--noise", nargs="?", const="off,kernel,torch", default=None,
                    help="with --policy: the exploration-noise legs (off, kernel, torch)")
    ap.add_argument("--population", nargs="?", const="a,b,c,d,e", default=None, help="with --policy: the population legs")
    ap.add_argument("--es", nargs="?", const="d,anti,plain,g8,grad", default=None,
                    help="with --policy: the ES perturbation legs (d, anti, plain, g8, grad)")
    ap.add_argument("--returns", action="store_true", help="returns and advantages against a torch loop")
    ap.add_argument("--policy-gradient", action="store_true", help="cp_policy_gradient against the torch update")
    ap.add_argument("--fp32-tflops", type=float, default=157.0, help="the fp32 vector peak for --policy-gradient's share")
    ap.add_argument("--tree", default=None, help="import cartpoleplusplus_amd from this checkout instead of the tool's own")
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="measured copy bandwidth for the weight-streaming floor")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ring", type=int, default=1 << 22)
    ap.add_argument("--sample", type=int, default=65536)
    args = ap.parse_args()
    if args.returns:
        return returns_bench(args)
    if args.policy_gradient:
        return policy_gradient_bench(args)
    if args.policy and args.es:
        return es_bench(args)
    if args.policy and args.population:
        return population_bench(args)
    if args.policy and args.noise:
        return noise_bench(args)
    if args.policy:
        return policy_bench(args)
    B, K, R = args.batch, args.steps, 3
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    acts = torch.randint(0, 5, (K, B, 2), dtype=torch.int8, device=dev, generator=g)
    out = {"batch": B, "steps": K}

    env = BatchedCartpole(B, 0, action_repeats=R, initial_force=55.0, autoreset=True, seed=1234)
    env.reset()
    for t in range(20):
        env.step(acts[t])
    out["base_ms"] = timed(lambda t: env.step(acts[t]), K)

    env.enable_lqr(torch.from_numpy(exact_gains()), state8=True)
    for t in range(20):
        env.step(acts[t])
    out["lqr_ms"] = timed(lambda t: env.step(acts[t]), K)
    env.enable_lqr(None)

    rm = ReplayMemory(args.ring, (R, 2, 7), 2, 1.5, num_envs=B)
    env.reset()
    rm.after_reset(env)

    def ingest(t):
        env.step(acts[t])
        rm.after_step(env, acts[t])
    for t in range(20):
        ingest(t)
    out["ingest_ms"] = timed(ingest, K)
    out["ingest_extra_ms"] = out["ingest_ms"] - out["base_ms"]
    rm.check()
    n = args.sample
    out["sample_n"] = n
    out["sample_ms"] = timed(lambda t: rm.sample(n), K)
    D = R * 2 * 7
    # per sample: 2 slot reads (8) + 2 f16 state rows read + written + action/reward/mask + idx
    sample_bytes = n * (8 + 4 * D * 2 + 2 * (2 * 4 + 4 + 4) + 4)
    out["sample_GBps"] = sample_bytes / (out["sample_ms"] * 1e-3) / 1e9
    out["replay_size"] = rm.size()
    out["env_steps_per_s"] = {k: B / (out[k + "_ms"] * 1e-3) for k in ("base", "lqr", "ingest")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
