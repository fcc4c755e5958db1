"""numpy restatement of cp_returns_compute's contract (include/cartpole_amd.h: cp_returns).

The raw kinds run in float32 with every product and sum rounded on its own: a loop over k, vectorised over the B
envs.  Standardisation runs in float64 with math.fsum (exactly rounded sums), per population member."""
import math

import numpy as np

EPISODE_TOTAL, DISCOUNTED, GAE = "episode_total", "discounted", "gae"
SAME_STEP, STICKY, NEXT_STEP = "same_step", "sticky", "next_step"
KINDS = (EPISODE_TOTAL, DISCOUNTED, GAE)
BOUNDARIES = (SAME_STEP, STICKY, NEXT_STEP)
f32 = np.float32


def padding(done, boundary, done_in=None):
    """(K, B) bool: the samples that are steps of no episode."""
    d = np.asarray(done) != 0
    K, B = d.shape
    din = np.zeros(B, bool) if done_in is None else np.asarray(done_in) != 0
    pad = np.zeros((K, B), bool)
    if boundary == STICKY:
        seen = din.copy()
        for k in range(K):
            pad[k] = seen
            seen = seen | d[k]
    elif boundary == NEXT_STEP:
        pad[0] = din
        pad[1:] = d[:-1]
    elif boundary != SAME_STEP:
        raise ValueError(boundary)
    return pad


def raw(reward, done, kind=EPISODE_TOTAL, boundary=SAME_STEP, gamma=1.0, lam=1.0, values=None, head=None,
        done_in=None, tail=None, mask_open=False):
    """-> adv (K, B) float32, valid (K, B) uint8, carry (B,) float32, ret (K, B) float32 or None."""
    r = np.asarray(reward, f32)
    d = np.asarray(done) != 0
    K, B = r.shape
    pad = padding(d, boundary, done_in)
    adv = np.zeros((K, B), f32)
    valid = np.zeros((K, B), bool)
    carry = np.zeros(B, f32)
    ret = None
    if kind == EPISODE_TOTAL:
        T = np.zeros(B, f32)
        if head is not None:
            T = np.where(pad[0], f32(0), np.asarray(head, f32)).astype(f32)
        closing = np.zeros((K, B), f32)
        is_open = np.zeros(B, bool)
        for k in range(K):
            step = ~pad[k]
            T = np.where(step, T + r[k], T).astype(f32)
            close = step & d[k]
            closing[k] = np.where(close, T, f32(0))
            T = np.where(close, f32(0), T).astype(f32)
            is_open = step & ~d[k]
        carry = np.where(is_open, T, f32(0)).astype(f32)
        cur = np.zeros(B, f32)
        closed = np.zeros(B, bool)
        for k in range(K - 1, -1, -1):
            close = ~pad[k] & d[k]
            closed = np.where(pad[k], False, closed | close)
            cur = np.where(close, closing[k], cur).astype(f32)
            valid[k] = closed
            adv[k] = np.where(closed, cur, f32(0))
        return adv, valid.astype(np.uint8), carry, ret
    g = f32(gamma)
    still_open = np.ones(B, bool)
    if kind == DISCOUNTED:
        G = np.zeros(B, f32) if tail is None else np.asarray(tail, f32).copy()
        for k in range(K - 1, -1, -1):
            step = ~pad[k]
            still_open = still_open & step & ~d[k]
            G = np.where(d[k], r[k], r[k] + (g * G).astype(f32)).astype(f32)
            G = np.where(step, G, f32(0)).astype(f32)
            valid[k] = step & ~(mask_open & still_open)
            adv[k] = np.where(valid[k], G, f32(0))
    elif kind == GAE:
        V = np.asarray(values, f32)
        assert V.shape == (K + 1, B)
        c = f32(g * f32(lam))
        A = np.zeros(B, f32)
        ret = np.zeros((K, B), f32)
        for k in range(K - 1, -1, -1):
            step = ~pad[k]
            still_open = still_open & step & ~d[k]
            delta = ((r[k] + (g * V[k + 1]).astype(f32)).astype(f32) - V[k]).astype(f32)
            A = np.where(d[k], (r[k] - V[k]).astype(f32), (delta + (c * A).astype(f32)).astype(f32)).astype(f32)
            A = np.where(step, A, f32(0)).astype(f32)
            valid[k] = step & ~(mask_open & still_open)
            adv[k] = np.where(valid[k], A, f32(0))
            ret[k] = np.where(valid[k], (A + V[k]).astype(f32), f32(0))
    else:
        raise ValueError(kind)
    return adv, valid.astype(np.uint8), carry, ret


def members(B, env_id_offset=0, population=1, group=1):
    """(B,) int64: the population member of each env of a call."""
    if population <= 1:
        return np.zeros(B, np.int64)
    return np.array([((int(env_id_offset) + i) // int(group)) % int(population) for i in range(B)], np.int64)


def standardise(adv, valid, env_id_offset=0, population=1, group=1):
    """util.standardise per member, float64 with exactly rounded sums.
    -> out (K, B) float32, stats (P, 4) float64 (n, mean, std, degenerate)."""
    x = np.asarray(adv, f32)
    v = np.asarray(valid) != 0
    K, B = x.shape
    P = max(int(population), 1)
    mem = members(B, env_id_offset, population, group)
    out = np.zeros((K, B), f32)
    stats = np.zeros((P, 4), np.float64)
    stats[:, 3] = 1.0
    for m in np.unique(mem):
        sel = v & (mem == m)[None, :]
        xs = x[sel].astype(np.float64)
        n = xs.size
        if n == 0:
            continue
        mean = math.fsum(xs) / n
        std = math.sqrt(math.fsum((xs - mean) ** 2) / n)
        degenerate = std == 0.0
        stats[m] = (n, mean, std, 1.0 if degenerate else 0.0)
        if not degenerate:
            out[sel] = ((xs - mean) / std).astype(f32)
    return out, stats


def standardise_bound(ref_out, adv, valid, stats, mem):
    """The bound on |out - ref| per sample: 2^-24 |ref| + 2 E, E = n 2^-52 (max|x| + |mean|) / std (1 + |ref|):
    the float32 rounding of the fp64 quotient plus an over-bound of the fp64 summation error of any order."""
    x = np.abs(np.asarray(adv, np.float64))
    v = np.asarray(valid) != 0
    bound = np.zeros(x.shape, np.float64)
    for m in np.unique(mem):
        n, mean, std, deg = stats[m]
        if deg:
            continue
        sel = v & (mem == m)[None, :]
        E = n * 2.0 ** -52 * (x[sel].max() + abs(mean)) / std * (1.0 + np.abs(ref_out[sel].astype(np.float64)))
        bound[sel] = 2.0 ** -24 * np.abs(ref_out[sel].astype(np.float64)) + 2.0 * E
    return bound
