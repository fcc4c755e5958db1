"""numpy restatement of the in-kernel MLP policy's arithmetic (include/cartpole_amd.h: cp_policy),
independent of the product code and with no compile step.

The contract fixes every fp32 rounding: acc = b[j], then acc = fmaf(W[j][i], x[i], acc) for i ascending.
numpy has no fused multiply-add, so `fmaf` emulates it exactly: the product of two float32 is exact in
float64 (48 significant bits), TwoSum gives the float64 sum's error term, and the one case where rounding
that float64 sum to float32 differs from rounding the exact value -- the sum sits on a float32 tie and the
error term is not zero -- is moved off the tie by one float64 ulp in the error's direction first.
"""
import numpy as np

TANH, CLIP, ARGMAX, SAMPLE = range(4)
SAMPLE_CTR0 = 0x40000000
DELTA = 2.0 ** -18


def fmaf(a, b, c):
    """round_f32(a * b + c) with one rounding, elementwise over float32 arrays."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)   # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                  # TwoSum: p + c64 = s + err exactly
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)                       # exact
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf))
        gap = np.nextafter(r, toward).astype(np.float64) - r.astype(np.float64)
        tie = np.isfinite(s) & (d != 0) & (2.0 * d == gap) & (err != 0)
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def forward(layers, x):
    """The last layer's linear outputs z (B, out) float32 for x (B, in) float32; layers [(W (out, in), b (out,))]."""
    x = np.ascontiguousarray(x, np.float32)
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).copy()
        for i in range(W.shape[1]):
            acc = fmaf(W[None, :, i], x[:, i, None], acc)
        x = np.where(acc > 0, acc, np.float32(0)).astype(np.float32) if k + 1 < len(layers) else acc
    return x


def act_clip(z, noise=None):
    n = np.zeros_like(z) if noise is None else np.asarray(noise, np.float32).reshape(z.shape)
    return np.minimum(np.maximum((z + n).astype(np.float32), np.float32(-1)), np.float32(1)).reshape(-1, 2, 2)


def act_argmax(z):
    return np.argmax(z.reshape(-1, 2, 5), axis=2).astype(np.int8)   # the first of equal maxima


def sample_words(steps, episode, gid, seed):
    """(B, 2, 4) uint32: per env and cart c, Philox4x32-10(ctr = (0x40000000 + 2 steps + c, episode, gid_lo,
    gid_hi), key = seed)."""
    from oracle import oracle as O
    steps, episode, gid = np.asarray(steps), np.asarray(episode), np.asarray(gid)
    w = np.zeros((len(steps), 2, 4), np.uint32)
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    for i in range(len(steps)):
        g = int(gid[i]) & 0xFFFFFFFFFFFFFFFF
        for c in range(2):
            ctr = ((SAMPLE_CTR0 + 2 * int(steps[i]) + c) & 0xFFFFFFFF, int(episode[i]) & 0xFFFFFFFF,
                   g & 0xFFFFFFFF, g >> 32)
            w[i, c] = O.philox4x32_10(ctr, key)
    return w


def check_sample(z, actions, words, epsilon, delta=DELTA):
    """The SAMPLE head's draws against the float64 reference.  Returns (number of epsilon draws, number of
    softmax draws, the fraction of softmax draws within delta of an interior boundary in the reference);
    raises AssertionError on a draw the contract does not allow."""
    z = np.asarray(z, np.float32).reshape(-1, 2, 5)
    a = np.asarray(actions).reshape(-1, 2).astype(np.int64)
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    eps_draw = u[..., 0] < np.float32(epsilon)
    a_eps = ((words[..., 1] >> np.uint32(8)).astype(np.uint64) * np.uint64(5)) >> np.uint64(24)
    assert np.array_equal(a[eps_draw], a_eps[eps_draw].astype(np.int64)), "epsilon draws"
    z64 = z.astype(np.float64)
    e = np.exp(z64 - z64.max(axis=2, keepdims=True))
    Cum = np.cumsum(e, axis=2)
    t = u[..., 2].astype(np.float64) * Cum[..., 4]
    lo = np.where(a > 0, np.take_along_axis(Cum, np.maximum(a - 1, 0)[..., None], 2)[..., 0], 0.0)
    hi = np.take_along_axis(Cum, a[..., None], 2)[..., 0]
    ok = (lo * (1 - delta) <= t) & ((t < hi * (1 + delta)) | (a == 4))
    bad = ~eps_draw & ~ok
    assert not bad.any(), f"{int(bad.sum())} softmax draws outside their interval, first at {np.argwhere(bad)[0]}"
    near = (np.abs(t[..., None] - Cum[..., :4]) <= delta * Cum[..., :4]).any(axis=2) & ~eps_draw
    n_soft = int((~eps_draw).sum())
    return int(eps_draw.sum()), n_soft, float(near.sum()) / max(n_soft, 1)


def random_layers(rng, widths, scale=1.0):
    """Random float32 layers [(W, b)] for widths (in, h1, .., out), W ~ N(0, scale / sqrt(in))."""
    out = []
    for nin, nout in zip(widths[:-1], widths[1:]):
        out.append(((rng.standard_normal((nout, nin)) * scale / np.sqrt(nin)).astype(np.float32),
                    (rng.standard_normal(nout) * 0.1).astype(np.float32)))
    return out


def packed(layers):
    """The C-ABI's weight layout: per layer W[out][in] row-major, then b[out]."""
    return np.concatenate([np.concatenate([np.asarray(W, np.float32).reshape(-1), np.asarray(b, np.float32)])
                           for W, b in layers])
