"""numpy restatement of cp_policy_gradient's contract (include/cartpole_amd.h), independent of the product code.

z, every layer's activations and the ReLU masks come from the exact fp32 emulation of the forward pass
(policy_ref.fmaf, the arithmetic of policy_ref.forward layer by layer).  From those fp32 values the softmax, logp and
the whole backward pass run in float64: the exact derivative of the contract's function at the fp32 forward pass, so
no ReLU can flip between the reference and the kernel.

`absscale` is the same backward pass on absolute values (|coeff|, |dz| terms, |W|^T, |x|): per parameter, the sum
of the magnitudes of every term that enters it, which scales the first-order rounding bound of any summation
order.
"""
import numpy as np

from tests import policy_ref

U = 2.0 ** -24


def widths_of(layers):
    return [np.asarray(layers[0][0]).shape[1]] + [np.asarray(W).shape[0] for W, _ in layers]


def forward_acts(layers, x):
    """[x_0, x_1, .., z]: every layer's input (float32, post-ReLU) and the last layer's linear output."""
    x = np.ascontiguousarray(x, np.float32)
    acts = [x]
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).copy()
        for i in range(W.shape[1]):
            acc = policy_ref.fmaf(W[None, :, i], x[:, i, None], acc)
        x = np.where(acc > 0, acc, np.float32(0)).astype(np.float32) if k + 1 < len(layers) else acc
        acts.append(x)
    return acts


def logp64(z, actions):
    """-> (logp (N,), lp (N, 2), D (N, 2) = max_j (m - z_j), p (N, 2, 5)) in float64 from float32 z (N, 10)."""
    z = np.asarray(z, np.float64).reshape(-1, 2, 5)
    a = np.asarray(actions).reshape(-1, 2).astype(np.int64)
    m = z.max(axis=2, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=2, keepdims=True)
    za = np.take_along_axis(z, a[..., None], 2)[..., 0]
    lp = (za - m[..., 0]) - np.log(S[..., 0])
    return lp.sum(axis=1), lp, (m - z).max(axis=2), e / S


def logp_bound(lp, D):
    """The header's fp32 arithmetic against float64: u * sum_c (12 + 2 D_c + 2 |lp_c|)."""
    return U * (12.0 + 2.0 * D + 2.0 * np.abs(lp)).sum(axis=1)


def evaluated(actions, coeff):
    a = np.asarray(actions).reshape(-1, 2)
    c = np.asarray(coeff, np.float32).reshape(-1)
    return (c != 0) & (a >= 0).all(axis=1) & (a < 5).all(axis=1)


def gradient(layers, x, actions, coeff):
    """One member's samples x (N, in), actions (N, 2), coeff (N,) -> dict(z float32 (N, 10) (0 where skipped),
    logp float64 (N,) (0 where skipped), lp, D, grad float64 (F,), absscale float64 (F,), n evaluated)."""
    x = np.ascontiguousarray(x, np.float32).reshape(len(x), -1)
    a = np.asarray(actions).reshape(-1, 2).astype(np.int64)
    c = np.asarray(coeff, np.float32).reshape(-1)
    ev = evaluated(a, c)
    N = len(x)
    F = sum(np.asarray(W).size + np.asarray(b).size for W, b in layers)
    out = dict(z=np.zeros((N, 10), np.float32), logp=np.zeros(N), lp=np.zeros((N, 2)), D=np.zeros((N, 2)),
               grad=np.zeros(F), absscale=np.zeros(F), n=int(ev.sum()), evaluated=ev)
    if not ev.any():
        return out
    acts = forward_acts(layers, x[ev])
    z = acts[-1]
    lpsum, lp, D, p = logp64(z, a[ev])
    out["z"][ev] = z
    out["logp"][ev] = lpsum
    out["lp"][ev] = lp
    out["D"][ev] = D
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, a[ev][..., None], 1.0, axis=2)
    c64 = c[ev].astype(np.float64)[:, None, None]
    delta = (c64 * (onehot - p)).reshape(-1, 10)
    dabs = (np.abs(c64) * (onehot + p)).reshape(-1, 10)
    parts, aparts = [], []
    for l in range(len(layers) - 1, -1, -1):
        W = np.asarray(layers[l][0], np.float64)
        xin = acts[l].astype(np.float64)
        parts.append(np.concatenate([(delta.T @ xin).reshape(-1), delta.sum(axis=0)]))
        aparts.append(np.concatenate([(dabs.T @ np.abs(xin)).reshape(-1), dabs.sum(axis=0)]))
        if l:
            mask = acts[l] > 0
            delta = np.where(mask, delta @ W, 0.0)
            dabs = np.where(mask, dabs @ np.abs(W), 0.0)
    out["grad"] = np.concatenate(parts[::-1])
    out["absscale"] = np.concatenate(aparts[::-1])
    return out


def grad_bound(widths, n, absscale):
    """(N_m + sum_{l >= 1} width[l] + 16) * u * absscale: the first-order bound for any summation order of the
    member's n evaluated samples plus the backward dot products."""
    return (n + sum(widths[1:]) + 16) * U * absscale


def members(B, population, group, env_id_offset):
    gid = int(env_id_offset) + np.arange(B, dtype=np.int64)
    return (gid // max(int(group), 1)) % max(int(population), 1)


def window(member_layers, obs, actions, coeff, population=1, group=1, env_id_offset=0):
    """The whole call: obs (K, B, in), actions (K, B, 2), coeff (K, B), member_layers a list of P layer lists ->
    dict(logits (K, B, 10) float32, logp (K, B) float64, bound_logp (K, B), grad (P, F), absscale (P, F), n (P,))."""
    K, B = coeff.shape
    P = max(int(population), 1)
    mem = members(B, P, group, env_id_offset) if P > 1 else np.zeros(B, np.int64)
    F = sum(np.asarray(W).size + np.asarray(b).size for W, b in member_layers[0])
    res = dict(logits=np.zeros((K, B, 10), np.float32), logp=np.zeros((K, B)), bound_logp=np.zeros((K, B)),
               grad=np.zeros((P, F)), absscale=np.zeros((P, F)), n=np.zeros(P, np.int64))
    obs = np.asarray(obs, np.float32).reshape(K, B, -1)
    for m in range(P):
        sel = mem == m
        if not sel.any():
            continue
        g = gradient(member_layers[m], obs[:, sel].reshape(-1, obs.shape[2]), np.asarray(actions)[:, sel].reshape(-1, 2),
                     np.asarray(coeff)[:, sel].reshape(-1))
        nb = int(sel.sum())
        res["logits"][:, sel] = g["z"].reshape(K, nb, 10)
        res["logp"][:, sel] = g["logp"].reshape(K, nb)
        res["bound_logp"][:, sel] = logp_bound(g["lp"], g["D"]).reshape(K, nb)
        res["grad"][m], res["absscale"][m], res["n"][m] = g["grad"], g["absscale"], g["n"]
    return res
