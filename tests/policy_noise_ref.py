"""numpy restatement of cp_policy_act's in-kernel exploration noise (include/cartpole_amd.h:
cp_policy_noise), independent of the product code and with no compile step.

The contract fixes the Philox counter, how the words become u1 and t (float32) and every float32 rounding
of the OU update and the clip; what lies between (logf, sqrtf, cosf, sinf and two products) is libm's, so
`gauss64` takes the float32 u1 and t as the contract forms them and computes the normals in float64.
"""
import numpy as np

OFF, GAUSSIAN, OU = range(3)
RESET_ON_EPISODE, CLIP_SYMMETRIC = 0x1, 0x2
NOISE_CTR0 = 0x80000000
TWO_PI_F32 = np.float32(6.283185307179586)
DELTA = 2.0 ** -18       # the project's bound for libm-based draws (tests/policy_ref.py)


def noise_words(steps, episode, gid, seed):
    """(B, 4) uint32: per env Philox4x32-10(ctr = (0x80000000 + steps, episode, gid_lo, gid_hi), key = seed)."""
    from oracle import oracle as O
    steps, episode, gid = np.asarray(steps), np.asarray(episode), np.asarray(gid)
    w = np.zeros((len(steps), 4), np.uint32)
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    for i in range(len(steps)):
        g = int(gid[i]) & 0xFFFFFFFFFFFFFFFF
        ctr = ((NOISE_CTR0 + int(steps[i])) & 0xFFFFFFFF, int(episode[i]) & 0xFFFFFFFF, g & 0xFFFFFFFF, g >> 32)
        w[i] = O.philox4x32_10(ctr, key)
    return w


def uniforms(words):
    """(u1, t), float32 (B, 2) each, for q = 0, 1: u1 = (float)((w[2q] >> 8) + 1) * 2^-24 in (0, 1],
    t = 6.283185307179586f * ((float)(w[2q+1] >> 8) * 2^-24)."""
    w = np.asarray(words, np.uint32).reshape(-1, 4)
    u1 = ((w[:, 0::2] >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (w[:, 1::2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u1, (TWO_PI_F32 * u2).astype(np.float32)


def gauss64(words):
    """-> (g, r), float64 (B, 4) each: the four Box-Muller normals per env (component c for a00 a01 a10 a11) and
    the radius each one was scaled by.  u1 and t are float32 as in the contract, everything after is float64."""
    u1, t = uniforms(words)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t = t.astype(np.float64)
    g = np.empty((u1.shape[0], 4), np.float64)
    g[:, 0::2] = r * np.cos(t)
    g[:, 1::2] = r * np.sin(t)
    return g, np.repeat(r, 2, axis=1)


def clip(x, flags, max_magnitude):
    """Step 6: nothing for max_magnitude <= 0; by default min(x, max) (util.py:155 bounds from above only);
    CLIP_SYMMETRIC: min(max(x, -max), max)."""
    x = np.asarray(x, np.float32)
    m = np.float32(max_magnitude)
    if not m > 0:
        return x
    if flags & CLIP_SYMMETRIC:
        x = np.maximum(x, -m)
    return np.minimum(x, m)


def ou_update(x, n, theta, flags, max_magnitude, steps):
    """One OU step of the state rows x (B, 4) float32 with n = float32(sigma * g) (B, 4) float32:
    x = 0 where RESET_ON_EPISODE and steps == 0; x = x + theta * (-x); x = x + n; the clip.  Every product and
    sum is one float32 operation, as in the contract."""
    x = np.array(x, np.float32).reshape(-1, 4)
    n = np.asarray(n, np.float32).reshape(-1, 4)
    if flags & RESET_ON_EPISODE:
        x[np.asarray(steps).reshape(-1) == 0] = np.float32(0)
    pull = np.float32(theta) * (-x)
    assert pull.dtype == np.float32
    x = x + pull
    x = x + n
    assert x.dtype == np.float32
    return clip(x, flags, max_magnitude)
