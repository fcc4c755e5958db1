"""numpy restatement of the seeded ES perturbations (include/cartpole_amd.h: cp_policy_es), independent of the
product code and with no compile step.

The contract fixes every step: the Philox counter, the byte sum, and the three float32 roundings (eps, d, W').
`philox` is Philox4x32-10 over arrays of counters; tests/test_policy_es_cpu.py checks it word for word against
oracle.philox4x32_10, which the other restatements call one block at a time.
"""
import numpy as np

OFF, BYTES4 = range(2)
ANTITHETIC = 0x1
ES_CTR0 = 0xC0000000
K = np.float32(21845.0 ** -0.5)          # the float32 nearest to 21845^(-1/2)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) (broadcastable integer arrays) under key = seed (64 bits):
    uint32 words (..., 4)."""
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo32]
    return np.stack(c, axis=-1).astype(np.uint32)


def member_draw(members, flags):
    """(e, s): the draw index (uint64) and the sign (+1 / -1, float32) of each member."""
    m = np.asarray(members, np.uint64)
    if flags & ANTITHETIC:
        return m >> np.uint64(1), np.where(m & np.uint64(1), np.float32(-1), np.float32(1)).astype(np.float32)
    return m, np.ones(m.shape, np.float32)


def es_words(draws, F, seed=0, generation=0):
    """(len(draws), F) uint32: parameter f's word w[f & 3] of Philox4x32-10(ctr = (0xC0000000 + (f >> 2),
    generation, e_lo, e_hi), key = seed)."""
    e = np.asarray(draws, np.uint64).reshape(-1, 1)
    blk = np.arange((F + 3) // 4, dtype=np.uint64)[None, :]
    w = philox(ES_CTR0 + blk, generation, e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), seed)
    return w.reshape(e.shape[0], -1)[:, :F]


def epsilon_of_words(w):
    """eps = ((float)S - 510.0f) * K, S the sum of the word's four bytes; float32, one rounding (the product)."""
    w = np.asarray(w, np.uint32)
    S = sum((w >> np.uint32(8 * b)) & np.uint32(0xFF) for b in range(4))
    eps = (S.astype(np.float32) - np.float32(510.0)) * K
    assert eps.dtype == np.float32
    return eps


def es_epsilon(members, F, seed=0, generation=0, flags=ANTITHETIC):
    """(len(members), F) float32: eps(e(m), f), without the sign."""
    e, _ = member_draw(members, flags)
    return epsilon_of_words(es_words(e, F, seed, generation))


def es_delta(members, F, sigma, seed=0, generation=0, flags=ANTITHETIC):
    """(len(members), F) float32: s * d, d = sigma * eps rounded once (the sign flip is exact)."""
    _, s = member_draw(members, flags)
    d = np.float32(sigma) * es_epsilon(members, F, seed, generation, flags)
    assert d.dtype == np.float32
    return d * s[:, None]


def es_weights(theta, members, sigma, seed=0, generation=0, flags=ANTITHETIC):
    """(len(members), F) float32: W' = theta + d for s = +1, theta - d for s = -1, rounded once."""
    theta = np.asarray(theta, np.float32).reshape(-1)
    w = theta[None, :] + es_delta(members, theta.size, sigma, seed, generation, flags)
    assert w.dtype == np.float32
    return w


def es_gradient64(coeff, lo, F, seed=0, generation=0, flags=ANTITHETIC):
    """(g64, scale): g64[f] = sum_m coeff[m - lo] s(m) eps(e(m), f) in float64 over the members lo .. lo + n - 1 (eps the
    contract's float32 value), and scale[f] = sum_m |coeff_m eps_m|, what a summation error bound multiplies."""
    c = np.asarray(coeff, np.float32).astype(np.float64).reshape(-1)
    members = lo + np.arange(c.size, dtype=np.int64)
    _, s = member_draw(members, flags)
    eps = es_epsilon(members, F, seed, generation, flags).astype(np.float64)
    terms = (c * s.astype(np.float64))[:, None] * eps
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-24: the relative error bound of k float32 roundings in a row."""
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def unpacked(row, widths):
    """A packed weight row [F] as policy_ref's layers [(W (out, in), b (out,))]."""
    out, o = [], 0
    for nin, nout in zip(widths[:-1], widths[1:]):
        out.append((row[o:o + nout * nin].reshape(nout, nin), row[o + nout * nin:o + nout * nin + nout]))
        o += nout * nin + nout
    assert o == row.size
    return out
